// The adapter skeleton (aria_hip/detail/Stage.hpp) against stubs of the few C-ABI symbols it calls: every stub appends to a
// call log, so the program links to neither library and needs no device. What it pins: the text of the exception, the
// destruction order of a class shaped like the adapters (handle before scratch buffer), that a constructor throwing after a
// successful create destroys the handle once, and DeviceScratch::reserve's sequence.
#include "aria_hip/detail/Stage.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {
std::vector<std::string> g_log;
const char* g_hip_error = "";
bool g_alloc_fails = false;
char g_blocks[4][16];
int g_next_block = 0;
}  // namespace

struct fake_stage_s { int alive; };
typedef fake_stage_s* fake_stage_t;

extern "C" {
const char* aria_status_string(int status) { return status == ARIA_E_NO_DEVICE ? "no usable HIP device" : status == ARIA_E_OOM ? "out of memory" : "other"; }
const char* aria_last_hip_error(void) { return g_hip_error; }
int aria_stream_synchronize(int, void*) { g_log.push_back("sync"); return ARIA_OK; }
int aria_device_alloc(int, size_t, void** d_ptr) {
    g_log.push_back("alloc");
    if (g_alloc_fails) return ARIA_E_OOM;
    *d_ptr = g_blocks[g_next_block++ % 4];
    return ARIA_OK;
}
int aria_device_free(int, void*) { g_log.push_back("free"); return ARIA_OK; }
int fake_create(fake_stage_t* out) {
    g_log.push_back("create");
    static fake_stage_s the_stage;
    *out = &the_stage;
    return ARIA_OK;
}
void fake_destroy(fake_stage_t) { g_log.push_back("destroy"); }
}

namespace {
using namespace aria::adapters::hip;

int g_failed = 0;
void check(bool ok, const char* what) {
    if (ok) return;
    std::printf("FAILED: %s\n", what);
    g_failed++;
}
std::string joined() {
    std::string s;
    for (const std::string& e : g_log) s += (s.empty() ? "" : " ") + e;
    return s;
}
// the parent's per-class fail(), as every adapter had it
std::string parentMessage(const char* cls, const char* where, int status) {
    std::string msg = std::string(cls) + ": " + where + ": " + aria_status_string(status);
    const char* hip = aria_last_hip_error();
    if (hip && hip[0]) msg += std::string(" [") + hip + "]";
    return msg;
}
std::string thrownBy(const char* cls, const char* where, int status) {
    try {
        detail::expect(cls, where, status);
    } catch (const std::runtime_error& e) {
        return e.what();
    }
    return "<nothing thrown>";
}

// Shaped like the adapters that have both: the scratch buffer declared before the handle.
class Adapter {
public:
    explicit Adapter(bool throw_after_create = false) : scratch_("Adapter", 0) {
        detail::expect("Adapter", "fake_create", fake_create(h_.out()));
        if (throw_after_create) detail::fail("Adapter", "validation", ARIA_E_INVALID);
    }
    void use(std::size_t bytes) { scratch_.reserve(nullptr, bytes); }
    const detail::DeviceScratch& scratch() const { return scratch_; }

private:
    detail::DeviceScratch scratch_;
    detail::StageOwner<fake_stage_t, fake_destroy> h_;
};
}  // namespace

int main() {
    // the message, byte for byte, without and with a HIP error string
    check(thrownBy("HipObjectDetector", "aria_det_create", ARIA_E_NO_DEVICE) == "HipObjectDetector: aria_det_create: no usable HIP device",
          "message without a HIP error");
    check(thrownBy("HipMapper", "aria_map_size", ARIA_E_NO_DEVICE) == parentMessage("HipMapper", "aria_map_size", ARIA_E_NO_DEVICE),
          "message equals the parent's format");
    g_hip_error = "hipErrorNoDevice";
    check(thrownBy("HipMapper", "aria_map_size", ARIA_E_HIP) == "HipMapper: aria_map_size: other [hipErrorNoDevice]", "message with a HIP error");
    check(thrownBy("HipMapper", "aria_map_size", ARIA_E_HIP) == parentMessage("HipMapper", "aria_map_size", ARIA_E_HIP),
          "message with a HIP error equals the parent's format");
    check(thrownBy("HipMapper", "aria_map_size", ARIA_OK) == "<nothing thrown>", "expect is silent on ARIA_OK");
    g_hip_error = "";

    // destruction: the handle (which drains the stream) before the buffer the stream reads
    g_log.clear();
    {
        Adapter a;
        a.use(100);
    }
    check(joined() == "create sync alloc destroy free", "destroy before device_free");

    // a constructor that throws after a successful create
    g_log.clear();
    bool threw = false;
    try {
        Adapter a(true);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    check(threw && joined() == "create destroy", "one destroy when the constructor throws after create");

    // reserve: synchronise, free, alloc only when growing
    g_log.clear();
    {
        detail::DeviceScratch s("Adapter", 0);
        s.reserve(nullptr, 0);
        check(g_log.empty() && !s.data() && s.capacity() == 0, "reserve(0) of an empty buffer does nothing");
        s.reserve(nullptr, 64);
        check(joined() == "sync alloc" && s.data() && s.capacity() == 64, "first reserve: sync, alloc (nothing to free)");
        g_log.clear();
        s.reserve(nullptr, 64);
        s.reserve(nullptr, 10);
        check(g_log.empty() && s.capacity() == 64, "no call when the capacity suffices");
        s.reserve(nullptr, 65);
        check(joined() == "sync free alloc" && s.capacity() == 65, "growing: sync, free, alloc");

        // a failing allocation: throws, the buffer is empty, and its destructor frees nothing
        g_log.clear();
        g_alloc_fails = true;
        std::string what;
        try {
            s.reserve(nullptr, 1000);
        } catch (const std::runtime_error& e) {
            what = e.what();
        }
        g_alloc_fails = false;
        check(what == "Adapter: aria_device_alloc: out of memory", "a failing alloc throws through fail");
        check(joined() == "sync free alloc" && !s.data() && s.capacity() == 0, "a failing alloc leaves pointer null and capacity 0");
        g_log.clear();
    }
    check(g_log.empty(), "the destructor after a failed alloc frees nothing");

    // the layout helper: 256-byte blocks
    detail::ScratchLayout l;
    check(l.take(1) == 0 && l.take(256) == 256 && l.take(257) == 512 && l.total == 1024, "ScratchLayout rounds every block up to 256 bytes");

    if (g_failed) return 1;
    std::printf("OK stage_skeleton\n");
    return 0;
}
