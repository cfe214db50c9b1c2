// What every adapter class over the C-ABI (include/aria_orb_hip.h) shares, and only what was identical in all of them: the
// exception a failing status becomes, the ownership of one stage handle, and one grow-only device allocation.
//
// DECLARATION ORDER. A class that has both a DeviceScratch and a StageOwner declares the DeviceScratch FIRST. Members are
// destroyed in reverse order of declaration (and bases after members), and the handle has to die first: aria_<stage>_destroy
// drains the stream, and until it has, work on that stream may still read the scratch buffer.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>

#include "aria_orb_hip.h"

namespace aria::adapters::hip::detail {

// "<Class>: <where>: <status string>", plus " [<hip error>]" when the HIP runtime left one
inline std::string message(const char* cls, const char* where, int status) {
    std::string msg = std::string(cls) + ": " + where + ": " + aria_status_string(status);
    const char* hip = aria_last_hip_error();
    if (hip && hip[0]) msg += std::string(" [") + hip + "]";
    return msg;
}

[[noreturn]] inline void fail(const char* cls, const char* where, int status) { throw std::runtime_error(message(cls, where, status)); }

inline void expect(const char* cls, const char* where, int rc) {
    if (rc != ARIA_OK) fail(cls, where, rc);
}

// One aria_<stage>_t, destroyed with its owner -- also when the owner's constructor throws after the create succeeded. A
// member, not a base: OrbHipExtractor and HipMatcher derive from the reference's ports.
template <class Handle, void (*Destroy)(Handle)>
class StageOwner {
public:
    StageOwner() = default;
    ~StageOwner() { reset(); }
    StageOwner(const StageOwner&) = delete;
    StageOwner& operator=(const StageOwner&) = delete;

    Handle get() const { return h_; }
    Handle* out() { return &h_; }             // where aria_<stage>_create writes; the owner is empty at that point
    void reset() {
        if (h_) Destroy(h_);
        h_ = nullptr;
    }

private:
    Handle h_ = nullptr;
};

// One grow-only device allocation. See DECLARATION ORDER above.
class DeviceScratch {
public:
    DeviceScratch(const char* cls, int device) : cls_(cls), device_(device) {}
    ~DeviceScratch() {
        if (p_) aria_device_free(device_, p_);
    }
    DeviceScratch(const DeviceScratch&) = delete;
    DeviceScratch& operator=(const DeviceScratch&) = delete;

    // At least `bytes` of capacity. Growing drains `stream` first: earlier work on it may still read the old block. A failed
    // allocation throws and leaves the buffer empty.
    void reserve(void* stream, std::size_t bytes) {
        if (bytes <= cap_) return;
        expect(cls_, "aria_stream_synchronize", aria_stream_synchronize(device_, stream));
        if (p_) aria_device_free(device_, p_);
        p_ = nullptr;
        cap_ = 0;
        expect(cls_, "aria_device_alloc", aria_device_alloc(device_, bytes, &p_));
        cap_ = bytes;
    }
    char* data() const { return static_cast<char*>(p_); }
    std::size_t capacity() const { return cap_; }
    int device() const { return device_; }

private:
    const char* cls_;
    int device_;
    void* p_ = nullptr;
    std::size_t cap_ = 0;
};

// Offsets of consecutive blocks in one scratch buffer, each rounded up to 256 bytes.
struct ScratchLayout {
    std::size_t total = 0;
    std::size_t take(std::size_t bytes) {
        const std::size_t at = total;
        total += (bytes + 255) / 256 * 256;
        return at;
    }
};

}  // namespace aria::adapters::hip::detail
