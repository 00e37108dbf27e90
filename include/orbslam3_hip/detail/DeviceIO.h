// orbslam3_hip/detail/DeviceIO.h — what the adapter headers share for moving data to and from the device: the return-code check, the two
// grow-only buffers, and the packed-block layout (256-byte aligned sections of one host staging block that mirrors one device block, so a
// call costs one host->device and one device->host transfer).
#ifndef ORBSLAM3_HIP_DETAIL_DEVICEIO_H
#define ORBSLAM3_HIP_DETAIL_DEVICEIO_H
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>

#include "../../orbhip.h"

namespace orbslam3_hip {
namespace detail {

inline void check(int rc, const char* what) { if (rc != ORB_OK) throw std::runtime_error(what); }

// device block that only ever grows; after a failed allocation it is empty (p == nullptr, cap == 0) and the next ensure() allocates again
struct DevBuf {
    void* p = nullptr; size_t cap = 0; int device = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) orb_dev_free(p); }
    void* ensure(size_t n) {
        if (n > cap) {
            if (p) orb_dev_free(p);
            p = nullptr; cap = 0;
            check(orb_dev_alloc(device, n, &p), "orb_dev_alloc");
            cap = n;
        }
        return p;
    }
    template <class T> T* upload(const T* h, size_t count) {
        T* d = (T*)ensure(count * sizeof(T) + 16);
        if (count) check(orb_memcpy_h2d(d, h, count * sizeof(T), nullptr), "orb_memcpy_h2d");
        return d;
    }
};
// page-locked host block (orb_host_alloc) with the same rules, grown by half more than asked for: the staging side of a packed block
struct HostBuf {
    uint8_t* p = nullptr; size_t cap = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { if (p) orb_host_free(p); }
    uint8_t* ensure(size_t n) {
        if (n > cap) {
            if (p) orb_host_free(p);
            p = nullptr; cap = 0;
            void* q = nullptr;
            check(orb_host_alloc(n + n / 2, &q), "orb_host_alloc");
            p = (uint8_t*)q; cap = n + n / 2;
        }
        return p;
    }
};

// One section of a packed block: `bytes` bytes of T at byte `offset`.  Layout hands them out 256-byte aligned in the order added; a
// zero-length section occupies nothing and shares its offset with the next one.
template <class T> struct Section { size_t offset, bytes; };
class Layout {
public:
    template <class T> Section<T> add(size_t count) {
        const Section<T> s{size_, count * sizeof(T)};
        size_ = (size_ + s.bytes + 255) & ~(size_t)255;
        return s;
    }
    size_t size() const { return size_; }
private:
    size_t size_ = 0;
};

// host data -> the staging block at section s (count <= the section's room)
template <class T> void put(const HostBuf& stage, Section<T> s, const T* h, size_t count) { std::memcpy(stage.p + s.offset, h, count * sizeof(T)); }
// the device address of section s in block d
template <class T> T* at(const DevBuf& d, Section<T> s) { return (T*)((uint8_t*)d.p + s.offset); }
// section s in a block downloaded from byte `from` (the offset of the first downloaded section) on
template <class T> const T* downloaded(const HostBuf& back, Section<T> s, size_t from) { return (const T*)(back.p + (s.offset - from)); }
// device -> host on `stream` (asynchronous: synchronise before reading); a failing copy throws here
inline void download(void* h, const void* d, size_t bytes, void* stream, const char* what = "orb_memcpy_d2h") { check(orb_memcpy_d2h(h, d, bytes, stream), what); }

}  // namespace detail
}  // namespace orbslam3_hip
#endif
