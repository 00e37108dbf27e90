// workspace.inc — the cursor a layout function walks a caller-allocated workspace with.  A workspace's sections are listed ONCE, in the layout
// function that fills the file's pointer struct; the final offset is the size, so *_workspace_bytes (which walks from a null base and reads no
// pointer: they are then bare offsets) and the entry point (or the kernel) share the one walk (DESIGN.md section 3).
#ifndef ORB_WORKSPACE_INC
#define ORB_WORKSPACE_INC
#include <cstddef>

struct WsCursor {
    unsigned char* base;   // nullptr: sizing only
    size_t align;          // every section is padded to a multiple of this (a power of two)
    size_t off;
    template <typename T> __host__ __device__ T* take(size_t count) {
        T* p = (T*)(base + off);   // (no null test: in a kernel it would cost a select per section)
        off += (count * sizeof(T) + align - 1) & ~(align - 1);
        return p;
    }
};
#endif
