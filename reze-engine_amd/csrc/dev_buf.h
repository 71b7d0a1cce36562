// dev_buf.h — the owners of a context's device memory (ctx.h). Every device array of a context is a member of one of these three types, so
// it is released when its owner is reset (`table = {}`), assigned or destroyed: there is no release list, and a new member cannot be
// forgotten. All three convert to T *, so a parameter block is filled (`p.geom = c->geom`) and a table tested (`if (!c->rj01)`) as with raw
// pointers. Nothing of the context in here: only the HIP allocator.
//   Scratch<T>  one allocation, move-only
//   Grown<T>    a Scratch with its capacity inside it, grown through grow() alone
//   Lent<T>     a table of RzStatic: owned where it was uploaded, and COPYING IT BORROWS
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>

namespace rzi {

// Device memory with one owner. As a local it is upload-time scratch, or a replacement under construction, released on every exit path
// (HIP_TRY returns early on failure); as a member it is released when its owner is reset or assigned (`owner = {}`).
template <class T> struct Scratch {
    T *p = nullptr;
    Scratch() = default;
    Scratch(Scratch &&o) noexcept : p(o.p) { o.p = nullptr; }
    Scratch &operator=(Scratch &&o) noexcept { std::swap(p, o.p); return *this; }       // (o goes out of scope with what this one held)
    ~Scratch() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t count) { return hipMalloc(&p, count * sizeof(T)); }
    operator T *() const { return p; }
};

// A grow-only array: the allocation and the element count it was made for travel together, so a capacity never describes another array
// than the one it stands beside. It changes through grow() below and by assignment.
template <class T> struct Grown {
    Grown() = default;
    Grown(Grown &&o) noexcept : a(std::move(o.a)), n(o.n) { o.n = 0; }
    Grown &operator=(Grown &&o) noexcept { a = std::move(o.a); std::swap(n, o.n); return *this; }
    size_t capacity() const { return n; }
    operator T *() const { return a.p; }
    T *get() const { return a.p; }      // (where the conversion must be spelled: `x ? a.get() : nullptr`, a reinterpret_cast)
    hipError_t alloc(size_t count)      // on an EMPTY array (a local replacement, a ring built anew): allocation and capacity in one step
    {
        const hipError_t e = a.alloc(count);
        if (e != hipSuccess) a.p = nullptr;
        n = a.p ? count : 0;
        return e;
    }
    // the request "hold `want` elements" that grow() takes, with room for the replacement
    struct To { Grown &arr; size_t want; Grown fresh; };
    To to(size_t want) { return To{ *this, want, Grown() }; }
private:
    Scratch<T> a;
    size_t n = 0;
};

// The one grow path, for one array or for arrays that grow as a set (the override table's three: physics relies on all of them keeping
// their addresses until all of them move). Nothing happens while every request fits. Otherwise every array of the set gets a replacement of
// at least its present capacity, and only when ALL of them are allocated does `drain` run — a buffer a frame may still read goes away
// behind a drain, and the caller says what draining is — and the arrays take their replacements and capacities together. On any failure
// every array, capacity and content is what it was. The contents do not move: what must be zeroed, re-armed or uploaded again after
// growing is the caller's to do.
template <class Drain, class... G> hipError_t grow(Drain &&drain, G &&...g)
{
    if (((g.want <= g.arr.capacity()) && ...)) return hipSuccess;
    hipError_t e = hipSuccess;
    ((e = e != hipSuccess ? e : g.fresh.alloc(std::max(g.want, g.arr.capacity()))), ...);
    if (e == hipSuccess) e = drain();
    if (e != hipSuccess) return e;
    ((g.arr = std::move(g.fresh)), ...);
    return hipSuccess;
}

// A device table of RzStatic. It owns its memory where it was uploaded; its COPY IS A BORROW — a non-owning alias of the same pointer,
// which frees nothing when it is reset or destroyed — and its move transfers ownership. That is rz_fork made a type: a fork borrows
// RzStatic by copying the struct. The lender outlives its forks (rz_destroy refuses while n_forks != 0) and neither side replaces a
// table while forks exist (static_unlocked). For members of RzStatic only: everything a context owns outright is move-only.
template <class T> struct Lent {
    Lent() = default;
    Lent(const Lent &o) : p(o.p), own(false) {}
    Lent(Lent &&o) noexcept : p(o.p), own(o.own) { o.p = nullptr; o.own = false; }
    Lent &operator=(const Lent &o) { if (this != &o) { release(); p = o.p; } return *this; }
    Lent &operator=(Lent &&o) noexcept { std::swap(p, o.p); std::swap(own, o.own); return *this; }
    ~Lent() { release(); }
    hipError_t alloc(size_t count)      // (on an empty table: an upload resets its table before it builds the new one)
    {
        release();
        const hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) p = nullptr;
        own = p != nullptr;
        return e;
    }
    operator T *() const { return p; }
    T *get() const { return p; }
private:
    T *p = nullptr;
    bool own = false;
    void release() { if (own && p) (void)hipFree(p); p = nullptr; own = false; }
};

}  // namespace rzi
