"""Place recognition on the device (include/aria_orb_hip.h, "place recognition"): a flat binary bag-of-words vocabulary trained
by k-majority clustering, the bags of frames, a ring database of bags and its scored top-K query. The reference has no such
code; aria_slam_amd.bow_ref is the definition and the device equals it bit for bit.

As with HipPoseEstimator, the handle's own stream is non-blocking: device buffers filled on torch's default stream must be
synchronised before a *_device call, or the index must be created on the caller's stream."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._handle import StageHandle
from ._lib import BOW_HIT_DTYPE, check
from .frontend import _ptr


def _frames_block(frames):
    """A list of [n_f, 32] uint8 arrays as one [F, stride, 32] block and its counts."""
    frames = [np.ascontiguousarray(f, np.uint8).reshape(-1, 32) for f in frames]
    stride = max([len(f) for f in frames] + [1])
    block = np.zeros((max(len(frames), 1), stride, 32), np.uint8)
    for k, f in enumerate(frames):
        block[k, :len(f)] = f
    return block, np.array([len(f) for f in frames], np.int32), stride


class HipBowIndex(StageHandle):
    """Binding of aria_bow_t. words: V that train() makes; rows: the most descriptors of a frame; capacity: entries kept (the
    oldest is dropped beyond it); top_k <= 32 hits per query; min_frames_between: the gate on query_id - id."""

    _prefix, _config = "bow", _lib.BowConfig

    def __init__(self, words=4096, rows=4096, capacity=65536, top_k=10, min_frames_between=30, train_iters=10, stream=None, device=0):
        cfg = self._default_config(device, stream)
        cfg.words, cfg.rows, cfg.capacity, cfg.top_k = words, rows, capacity, top_k
        cfg.min_frames_between, cfg.train_iters = min_frames_between, train_iters
        self._create(cfg)

    @property
    def words(self):
        """V of the vocabulary in use; 0 before there is one."""
        return self._L.aria_bow_words(self._h)

    @property
    def top_k(self):
        return self.config.top_k

    # ---- vocabulary
    def train(self, frames):
        """frames: a list of [n_f, 32] uint8 arrays. Blocks. Returns the iterations run."""
        block, counts, stride = _frames_block(frames)
        it = C.c_int(0)
        check(self._L.aria_bow_train(self._h, block.ctypes.data, counts.ctypes.data, len(counts), stride, C.byref(it)), "aria_bow_train")
        return it.value

    def train_device(self, d_desc, d_counts, n_frames, desc_stride):
        it = C.c_int(0)
        check(self._L.aria_bow_train_device(self._h, _ptr(d_desc), _ptr(d_counts), n_frames, desc_stride, C.byref(it)),
              "aria_bow_train_device")
        return it.value

    def vocabulary(self):
        """(words [V, 32] uint8, idf_q [V] uint16)."""
        V = self.words
        words, idf, n = np.zeros((max(V, 1), 32), np.uint8), np.zeros(max(V, 1), np.uint16), C.c_int(0)
        check(self._L.aria_bow_get_vocabulary(self._h, words.ctypes.data, idf.ctypes.data, C.byref(n)), "aria_bow_get_vocabulary")
        return words[:n.value], idf[:n.value]

    def set_vocabulary(self, words, idf_q):
        words = np.ascontiguousarray(words, np.uint8).reshape(-1, 32)
        idf = np.ascontiguousarray(idf_q, np.uint16).reshape(-1)
        if len(words) != len(idf):
            raise ValueError("one weight per word")
        check(self._L.aria_bow_set_vocabulary(self._h, words.ctypes.data, idf.ctypes.data, len(words)), "aria_bow_set_vocabulary")

    def save(self, path):
        check(self._L.aria_bow_save(self._h, os.fsencode(path)), "aria_bow_save")

    def load(self, path):
        check(self._L.aria_bow_load(self._h, os.fsencode(path)), "aria_bow_load")

    # ---- bags
    def transform_batch_device(self, d_desc, d_counts, n_frames, desc_stride, d_tf, d_norm):
        """aria_bow_transform_batch_device: device pointers (torch tensors or ints); d_tf holds n_frames * V uint16, d_norm
        n_frames int32. Enqueued on the handle's stream; check() synchronises and reports deferred errors."""
        check(self._L.aria_bow_transform_batch_device(self._h, _ptr(d_desc), _ptr(d_counts), n_frames, desc_stride, _ptr(d_tf),
                                                      _ptr(d_norm)), "aria_bow_transform_batch_device")

    # ---- database
    def add_batch_device(self, d_tf, d_norm, ids):
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        check(self._L.aria_bow_add_batch_device(self._h, _ptr(d_tf), _ptr(d_norm), ids.ctypes.data if len(ids) else None, len(ids)),
              "aria_bow_add_batch_device")

    def add(self, kf_id, descriptors):
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        check(self._L.aria_bow_add(self._h, int(kf_id), d.ctypes.data if len(d) else None, len(d)), "aria_bow_add")

    def add_device(self, kf_id, d_desc, n):
        check(self._L.aria_bow_add_device(self._h, int(kf_id), _ptr(d_desc), int(n)), "aria_bow_add_device")

    def size(self):
        return self._L.aria_bow_size(self._h)

    def info(self, index):
        """(id, norm) of entry `index`, oldest first."""
        kid, norm = C.c_longlong(0), C.c_int(0)
        check(self._L.aria_bow_info(self._h, index, C.byref(kid), C.byref(norm)), "aria_bow_info")
        return kid.value, norm.value

    # ---- queries
    def query_batch_device(self, d_tf, d_norm, query_ids, d_hits, d_counts):
        """d_hits: len(query_ids) * top_k BOW_HIT_DTYPE records on the device, d_counts: as many int32. Enqueued."""
        ids = np.ascontiguousarray(query_ids, np.int64).reshape(-1)
        check(self._L.aria_bow_query_batch_device(self._h, _ptr(d_tf), _ptr(d_norm), ids.ctypes.data if len(ids) else None, len(ids),
                                                  _ptr(d_hits), _ptr(d_counts)), "aria_bow_query_batch_device")

    def query(self, query_id, descriptors):
        """One frame from host descriptors; blocks. Returns (hits [top_k] BOW_HIT_DTYPE, count)."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        hits, n = np.zeros(self.top_k, BOW_HIT_DTYPE), C.c_int(0)
        check(self._L.aria_bow_query(self._h, int(query_id), d.ctypes.data if len(d) else None, len(d), hits.ctypes.data, C.byref(n)),
              "aria_bow_query")
        return hits, n.value

    def query_device(self, query_id, d_desc, n):
        """The same with the descriptors on the device."""
        hits, cnt = np.zeros(self.top_k, BOW_HIT_DTYPE), C.c_int(0)
        check(self._L.aria_bow_query_device(self._h, int(query_id), _ptr(d_desc), int(n), hits.ctypes.data, C.byref(cnt)),
              "aria_bow_query_device")
        return hits, cnt.value
