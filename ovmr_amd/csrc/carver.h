// Workspace layouts stated once (host only; not part of common.h, which holds what kernels are compiled from).
#pragma once
#include <stddef.h>

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// A workspace is one arena that every pass carves anew (calls on one handle are stream ordered).  Each pass states its buffers ONCE,
// as a Carver whose constructor takes them in order: on a null base that only measures (bytes() sizes the arena), on the arena it
// hands out the pointers the pass uses -- so a buffer cannot be sized without being carved, or the reverse.
struct Carver {
    char* base; size_t off = 0;
    explicit Carver(char* b) : base(b) {}
    template <typename T> T* take(size_t n) { T* p = base ? (T*)(base + off) : nullptr; off = align_up(off + n * sizeof(T)); return p; }
    size_t bytes() const { return off; }
};
