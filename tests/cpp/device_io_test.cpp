// include/orbslam3_hip/detail/DeviceIO.h on its own: the layout arithmetic, the growth rules of the two buffers, what a failed allocation leaves
// behind, the checked download.  Links no library: the eight runtime helpers of orbhip.h are defined here over malloc / memcpy, with call
// counters and switches that make the next allocation or the next device->host copy fail.  Built plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>

#include <orbslam3_hip/detail/DeviceIO.h>

static int g_devAlloc = 0, g_devFree = 0, g_hostAlloc = 0, g_hostFree = 0, g_h2d = 0, g_d2h = 0;
static size_t g_lastDevBytes = 0, g_lastHostBytes = 0;
static bool g_failAlloc = false, g_failD2h = false;

extern "C" {
int orb_dev_alloc(int, size_t bytes, void** p) {
    g_devAlloc++;
    if (g_failAlloc) { g_failAlloc = false; return ORB_E_HIP; }
    g_lastDevBytes = bytes;
    *p = std::malloc(bytes);
    return ORB_OK;
}
int orb_dev_free(void* p) { g_devFree++; std::free(p); return ORB_OK; }
int orb_host_alloc(size_t bytes, void** p) {
    g_hostAlloc++;
    if (g_failAlloc) { g_failAlloc = false; return ORB_E_HIP; }
    g_lastHostBytes = bytes;
    *p = std::malloc(bytes);
    return ORB_OK;
}
int orb_host_free(void* p) { g_hostFree++; std::free(p); return ORB_OK; }
int orb_memcpy_h2d(void* d, const void* h, size_t n, void*) { g_h2d++; std::memcpy(d, h, n); return ORB_OK; }
int orb_memcpy_d2h(void* h, const void* d, size_t n, void*) {
    g_d2h++;
    if (g_failD2h) { g_failD2h = false; return ORB_E_HIP; }
    std::memcpy(h, d, n);
    return ORB_OK;
}
int orb_memset(void* d, int v, size_t n, void*) { std::memset(d, v, n); return ORB_OK; }
int orb_stream_sync(void*) { return ORB_OK; }
}

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using namespace orbslam3_hip::detail;

template <class F> static std::string thrown(F f) {
    try { f(); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}

int main() {
    {   // layout: 256-byte aligned sections in the order added; a zero-length section occupies nothing; an empty layout has size 0
        Layout none;
        CHECK(none.size() == 0);
        Layout l;
        const auto a = l.add<int32_t>(3);      // 12 bytes
        const auto z = l.add<float>(0);        // nothing
        const auto b = l.add<uint8_t>(256);    // exactly one unit
        const auto c = l.add<double>(33);      // 264 bytes
        const auto z2 = l.add<uint8_t>(0);     // a zero-length section at the end
        CHECK(a.offset == 0 && a.bytes == 12);
        CHECK(z.offset == 256 && z.bytes == 0);
        CHECK(b.offset == 256 && b.bytes == 256);
        CHECK(c.offset == 512 && c.bytes == 264);
        CHECK(z2.offset == 1024 && z2.bytes == 0);
        CHECK(l.size() == 1024);
        Layout one;
        one.add<uint8_t>(1);
        CHECK(one.size() == 256);
    }
    {   // HostBuf: n + n / 2 bytes, no reallocation while n <= cap, never shrinks
        HostBuf h;
        uint8_t* p = h.ensure(1000);
        CHECK(p && h.cap == 1500 && g_lastHostBytes == 1500 && g_hostAlloc == 1);
        CHECK(h.ensure(1500) == p && h.ensure(1) == p && g_hostAlloc == 1 && h.cap == 1500);
        p = h.ensure(1501);
        CHECK(p && h.cap == 2251 && g_hostAlloc == 2 && g_hostFree == 1);
        // a failed allocation leaves the buffer empty, and the next ensure() allocates again
        g_failAlloc = true;
        CHECK(thrown([&] { h.ensure(5000); }) == "orb_host_alloc");
        CHECK(h.p == nullptr && h.cap == 0 && g_hostFree == 2);
        p = h.ensure(100);   // below the capacity before the failure
        CHECK(p && h.cap == 150 && g_hostAlloc == 4);
        std::memset(p, 0xAB, 150);
    }
    CHECK(g_hostFree == 3);
    {   // DevBuf: ensure(n) allocates n, upload(count) asks for count * sizeof(T) + 16, never shrinks
        DevBuf d;
        void* p = d.ensure(1000);
        CHECK(p && d.cap == 1000 && g_lastDevBytes == 1000 && g_devAlloc == 1);
        CHECK(d.ensure(1000) == p && d.ensure(8) == p && g_devAlloc == 1);
        const int32_t v[300] = {7, 8, 9};
        int32_t* q = d.upload(v, 300);
        CHECK(q && d.cap == 1216 && g_devAlloc == 2 && g_devFree == 1 && g_h2d == 1 && q[0] == 7 && q[2] == 9);
        CHECK(d.upload(v, 0) == q && g_h2d == 1 && g_devAlloc == 2);   // 0 elements: nothing is copied
        DevBuf empty;
        CHECK(empty.upload((const int32_t*)nullptr, 0) != nullptr && empty.cap == 16 && g_h2d == 1);
        g_failAlloc = true;
        CHECK(thrown([&] { d.ensure(4000); }) == "orb_dev_alloc");
        CHECK(d.p == nullptr && d.cap == 0);
        p = d.ensure(500);   // below the capacity before the failure
        CHECK(p && d.cap == 500);
        std::memset(p, 0xCD, 500);
        static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf owns its block");
        static_assert(!std::is_copy_constructible<HostBuf>::value && !std::is_copy_assignable<HostBuf>::value, "HostBuf owns its block");
    }
    CHECK(g_devAlloc == g_devFree + 1);   // every successful allocation was freed once (one allocation failed)
    {   // a packed block end to end: put, the typed device pointers, the download of a sub-range
        Layout l;
        const auto in = l.add<int32_t>(5);
        const auto skip = l.add<uint8_t>(0);
        const auto mid = l.add<double>(40);
        const auto out = l.add<int32_t>(70);
        HostBuf stage, back;
        DevBuf dev;
        stage.ensure(mid.offset);
        const int32_t src[5] = {1, 2, 3, 4, 5};
        put(stage, in, src, 5);
        dev.ensure(l.size());
        CHECK(orb_memcpy_h2d(dev.p, stage.p, mid.offset, nullptr) == ORB_OK);
        CHECK((uint8_t*)at(dev, in) == (uint8_t*)dev.p && (uint8_t*)at(dev, skip) == (uint8_t*)at(dev, mid));
        CHECK((uint8_t*)at(dev, mid) == (uint8_t*)dev.p + 256 && (uint8_t*)at(dev, out) == (uint8_t*)dev.p + 256 + 512);
        for (int i = 0; i < 40; i++) at(dev, mid)[i] = 0.5 * i;
        for (int i = 0; i < 70; i++) at(dev, out)[i] = at(dev, in)[i % 5] * 10 + i;
        const size_t len = out.offset + out.bytes - mid.offset;
        const int d2h = g_d2h;
        download(back.ensure(len), at(dev, mid), len, nullptr);
        CHECK(g_d2h == d2h + 1);
        CHECK((const uint8_t*)downloaded(back, mid, mid.offset) == back.p);
        CHECK((const uint8_t*)downloaded(back, out, mid.offset) == back.p + (out.offset - mid.offset));
        CHECK(downloaded(back, mid, mid.offset)[39] == 19.5 && downloaded(back, out, mid.offset)[69] == 5 * 10 + 69);
        // a failing copy throws at the copy, with the caller's text if it gave one
        g_failD2h = true;
        CHECK(thrown([&] { download(back.p, at(dev, mid), len, nullptr); }) == "orb_memcpy_d2h");
        g_failD2h = true;
        CHECK(thrown([&] { download(back.p, at(dev, mid), len, nullptr, "copy back failed"); }) == "copy back failed");
        CHECK(thrown([&] { check(ORB_OK, "fine"); }) == "" && thrown([&] { check(ORB_E_HIP, "broken"); }) == "broken");
    }
    std::printf("device_io_test OK\n");
    return 0;
}
