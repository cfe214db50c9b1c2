#!/usr/bin/env python3
"""Rates of the place-recognition stage (aria_bow_*) on one GPU, timed with HIP events on the handle's stream around
synchronised work, after a warm-up, the alternatives alternated in the same process, medians reported:

  training   V words from F frames x N descriptors: iterations run and wall time per iteration (the call blocks once per
             iteration); beside it the transform of the same frames (kNN-2 + histogram), which is what one iteration's quantising
             costs, so the difference is what the member lists and the majority pass add.
  transform  --frames frames x N descriptors at V words; beside it aria_matcher_match_batch_device on as many pairs of N x N.
  query      batches of 1, 64 and 1024 bags against databases of the --entries sizes: time, achieved bytes per second on the
             algorithmic bytes (entries x 2 roundup(V, 8) per tile of four queries) and their share of the 8 TB/s peak.
  loop       one query of N descriptors through aria_matcher_match_db_device over 500 keyframes, against transform + top-10 over
             65 536 bags + the exact check of 10 keyframes: what the feature exists for.

Descriptors are random words of a random vocabulary with a few flipped bits, so bags are as sparse as real ones. Prints one
JSON line; --out writes it to a file as well.

Usage: bow_rate.py [--words 4096] [--desc 2000] [--frames 4096] [--train-frames 256] [--entries 500,65536,1000000] [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8.0e12


def timed(torch, stream, fn, check, reps, warmup):
    for _ in range(warmup):
        fn()
    check()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    check()
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=4096)
    ap.add_argument("--desc", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--train-frames", type=int, default=256)
    ap.add_argument("--entries", default="500,65536,1000000")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import aria_slam_amd as A
    assert torch.cuda.is_available(), "bow_rate.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    V, N, B, F = a.words, a.desc, a.frames, a.train_frames
    Vp = (V + 7) & ~7
    sizes = [int(s) for s in a.entries.split(",")]
    batches = [int(s) for s in a.batches.split(",")]
    res = dict(words=V, descriptors=N, frames=B, train_frames=F, reps=a.reps)

    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    with torch.cuda.stream(stream):
        base = torch.randint(0, 256, (V, 32), dtype=torch.uint8, device=dev, generator=gen)
        pick = torch.randint(0, V, (B, N), device=dev, generator=gen)
        desc = base[pick]                                                                   # [B, N, 32]
        desc[:, :, 5] ^= torch.randint(0, 8, (B, N), dtype=torch.uint8, device=dev, generator=gen)
        counts = torch.full((B,), N, dtype=torch.int32, device=dev)
        tf = torch.zeros((B, V), dtype=torch.int16, device=dev)
        norm = torch.zeros((B,), dtype=torch.int32, device=dev)
    stream.synchronize()
    sync = stream.synchronize

    # ---- training
    ix = A.HipBowIndex(words=V, rows=max(N, 1), capacity=max(sizes), top_k=10, min_frames_between=0, stream=stream.cuda_stream)
    ix.train_device(desc, counts, F, N)                                                      # warm-up: buffers grow
    t = time.perf_counter()
    iters = ix.train_device(desc, counts, F, N)
    train_s = time.perf_counter() - t
    q_ms = timed(torch, stream, lambda: ix.transform_batch_device(desc, counts, F, N, tf, norm), ix.check, a.reps, a.warmup)
    res.update(train_iterations=iters, train_ms=train_s * 1e3, train_ms_per_iteration=train_s * 1e3 / (iters + 1),
               train_quantise_ms_median=q_ms[0], train_quantise_ms_min=q_ms[1], train_quantise_ms_max=q_ms[2])
    print("training %d words from %d x %d: %d iterations + the weights pass, %.2f ms = %.2f ms per pass; quantise + histogram alone "
          "%.3f ms (min %.3f max %.3f)" % (V, F, N, iters, train_s * 1e3, res["train_ms_per_iteration"], *q_ms))

    # ---- transform beside the matcher
    mat = A.HipMatcher(stream=stream.cuda_stream, max_query=max(N, 4096), max_train=max(N, 4096))
    with torch.cuda.stream(stream):
        m = torch.zeros((B, N, 12), dtype=torch.uint8, device=dev)
        nm = torch.zeros((B,), dtype=torch.int32, device=dev)
    sync()
    run_tf = lambda: ix.transform_batch_device(desc, counts, B, N, tf, norm)                  # noqa: E731
    run_mt = lambda: mat.match_batch_device(desc.data_ptr() + N * 32, counts.data_ptr() + 4, desc, counts, B - 1, N * 32, 0.75, m, nm, N)   # noqa: E731
    t_ms, m_ms = [], []
    for _ in range(3):                                                                        # alternated
        t_ms.append(timed(torch, stream, run_tf, ix.check, a.reps, a.warmup)[0])
        m_ms.append(timed(torch, stream, run_mt, sync, a.reps, a.warmup)[0])
    res.update(transform_ms=float(np.median(t_ms)), transform_ms_runs=t_ms, match_ms=float(np.median(m_ms)), match_ms_runs=m_ms,
               transform_over_match=float(np.median(t_ms) / np.median(m_ms)), bag_words_per_frame=float((tf[:64] != 0).sum(1).float().mean().item()))
    print("transform %d x %d at V = %d: %.3f ms; matcher on %d pairs of %d x %d: %.3f ms; ratio %.2f"
          % (B, N, V, res["transform_ms"], B - 1, N, N, res["match_ms"], res["transform_over_match"]))

    # ---- queries
    res["query"] = []
    filled = 0
    for size in sorted(sizes):
        while filled < size:                                                                 # the same bags again and again
            n = min(B, size - filled)
            ix.add_batch_device(tf, norm, np.arange(filled, filled + n))
            filled += n
        ix.check()
        assert ix.size() == size
        for nq in batches:
            nq = min(nq, B)
            with torch.cuda.stream(stream):
                hits = torch.zeros((nq, 10, 32), dtype=torch.uint8, device=dev)
                cnt = torch.zeros((nq,), dtype=torch.int32, device=dev)
            sync()
            qids = np.full(nq, 1 << 40, np.int64)
            reps = a.reps if size * nq <= (1 << 28) else 3
            ms = timed(torch, stream, lambda: ix.query_batch_device(tf, norm, qids, hits, cnt), ix.check, reps, 1)
            tiles = (nq + 3) // 4
            gbs = size * 2 * Vp * tiles / (ms[0] * 1e-3)
            row = dict(entries=size, queries=nq, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2], us_per_query=ms[0] * 1e3 / nq,
                       algorithmic_bytes_per_s=gbs, share_of_peak=gbs / PEAK_BYTES_PER_S, first_hits=int(cnt.min().item()))
            res["query"].append(row)
            print("query %7d entries x %4d queries: %.3f ms (min %.3f max %.3f), %.3f TB/s on the algorithmic bytes = %.1f %% of peak"
                  % (size, nq, ms[0], ms[1], ms[2], gbs / 1e12, 100 * gbs / PEAK_BYTES_PER_S))
        if size == 65536 or size == sorted(sizes)[-1] and "loop" not in res:
            # ---- the comparison the feature exists for
            rows = max(N, 1)
            with torch.cuda.stream(stream):
                kf = desc[:500].contiguous()
                kf_counts = counts[:500].contiguous()
                good = torch.zeros((500,), dtype=torch.int32, device=dev)
                sub, sub_counts = desc[:10].contiguous(), counts[:10].contiguous()
                good10 = torch.zeros((10,), dtype=torch.int32, device=dev)
                h1 = torch.zeros((1, 10, 32), dtype=torch.uint8, device=dev)
                c1 = torch.zeros((1,), dtype=torch.int32, device=dev)
            sync()
            one = np.full(1, 1 << 40, np.int64)

            def old():
                mat.match_db_device(desc[7], N, kf, kf_counts, 500, rows * 32, 0.7, good)

            def new():
                ix.transform_batch_device(desc[7], counts, 1, N, tf, norm)
                ix.query_batch_device(tf, norm, one, h1, c1)
                mat.match_db_device(desc[7], N, sub, sub_counts, 10, rows * 32, 0.7, good10)

            o_ms, n_ms = [], []
            for _ in range(3):
                o_ms.append(timed(torch, stream, old, sync, a.reps, a.warmup)[0])
                n_ms.append(timed(torch, stream, new, ix.check, a.reps, a.warmup)[0])
            res["loop"] = dict(entries=size, scan_500_ms=float(np.median(o_ms)), scan_500_ms_runs=o_ms, bow_top10_plus_check_ms=float(np.median(n_ms)),
                               bow_top10_plus_check_ms_runs=n_ms, larger="bow" if np.median(n_ms) > np.median(o_ms) else "scan")
            print("one query: exact scan of 500 keyframes %.3f ms; bag + top-10 of %d bags + exact check of 10 keyframes %.3f ms: the %s is larger"
                  % (res["loop"]["scan_500_ms"], size, res["loop"]["bow_top10_plus_check_ms"], "new path" if res["loop"]["larger"] == "bow" else "old scan"))
    ix.close()
    mat.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
