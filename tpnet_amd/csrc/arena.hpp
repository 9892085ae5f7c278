// Where a caller-owned buffer's layout lives.  Every such buffer has ONE layout function, a walk over its fields in order:
//     static void neg_layout(Arena& a, NegView& v, int64_t E) { a.head(); v.hdr = a.take<uint32_t>(64); ... }
// Walked by an Arena without a buffer it MEASURES (the *_bytes export is a.off afterwards; every pointer comes out null), walked by
// one with a buffer it PLACES the fields -- so a size and the pointers it has to cover cannot disagree.  Fields are 256-byte
// aligned.  A placing walk never gets ahead of the measuring one (head() costs it at most 255 bytes, the measure 256; every other
// step is the same), so a buffer of the measured size holds every field whatever its alignment.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tpnet {

static inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// workgroups of 256 threads that cover n items, at least one, at most cap
static inline int grid_1d(int64_t n, int cap) {
    const int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

struct Arena {
    struct Span { void* ptr; size_t bytes; };
    char* base = nullptr;          // null: measuring
    size_t bytes = 0;              // placing: the buffer's size (unknown to a caller that only reads the fields: nothing fits)
    size_t off = 0;                // bytes walked so far

    Arena() {}
    Arena(void* buf, size_t n) : base((char*)buf), bytes(n) {}
    // the buffer may start anywhere: placing rounds the base up to 256, measuring sets aside the 256 bytes this may cost
    void head() { off = base ? align256((size_t)base + off) - (size_t)base : off + 256; }
    template <class T> T* take(size_t count) {
        T* r = base ? (T*)(base + off) : nullptr;
        off += align256(count * sizeof(T));
        return r;
    }
    // bytes no field uses: slack and spare slots that keep a size what it has been
    void skip(size_t n) { off += align256(n); }
    // everything from here to the end of the buffer: what a rocPRIM call gets as its temporary storage
    Span rest() const { return {base ? base + off : nullptr, base && off < bytes ? bytes - off : 0}; }
    bool fits() const { return off <= bytes; }
};

// the size a layout measures: layout(a) walks an Arena without a buffer
template <class Layout> static size_t measured(Layout layout) {
    Arena a;
    layout(a);
    return a.off;
}

}  // namespace tpnet
