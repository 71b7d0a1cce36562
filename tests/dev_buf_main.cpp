// The owners of a context's device memory (reze-engine_amd/csrc/dev_buf.h) on the CPU: this program includes only that header and defines
// hipMalloc / hipFree itself, backed by malloc, with a count of live blocks and a switch that fails the n-th allocation. No HIP library
// is linked. One "ok" line per case; the first failure exits non-zero. Built and run by tests/test_dev_buf_cpu.py under ASan and UBSan.
#include "../reze-engine_amd/csrc/dev_buf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static int g_live = 0, g_allocs = 0, g_frees = 0;
static int g_fail_at = 0;               // the n-th allocation from now fails (1 = the next one); 0 = none

extern "C" hipError_t hipMalloc(void **ptr, size_t size)
{
    if (g_fail_at && --g_fail_at == 0) { *ptr = nullptr; return hipErrorOutOfMemory; }
    *ptr = malloc(size ? size : 1);
    if (!*ptr) return hipErrorOutOfMemory;
    ++g_live; ++g_allocs;
    return hipSuccess;
}

extern "C" hipError_t hipFree(void *ptr)
{
    if (ptr) { free(ptr); --g_live; ++g_frees; }
    return hipSuccess;
}

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

using rzi::Grown;
using rzi::Lent;
using rzi::Scratch;

static int g_drains = 0;
static hipError_t drained() { ++g_drains; return hipSuccess; }

static void release_by_reset_and_scope()
{
    {
        Scratch<float> s;
        CHECK(s.alloc(16) == hipSuccess && s.p && g_live == 1);
        s = {};
        CHECK(!s.p && g_live == 0);
        CHECK(s.alloc(4) == hipSuccess);
        Grown<int> g;
        CHECK(rzi::grow(drained, g.to(8)) == hipSuccess && g_live == 2);
        g = {};
        CHECK(!g && g.capacity() == 0 && g_live == 1);
        CHECK(rzi::grow(drained, g.to(8)) == hipSuccess);
        Lent<uint32_t> l;
        CHECK(l.alloc(32) == hipSuccess && g_live == 3);
        l = {};
        CHECK(!l && g_live == 2);
        CHECK(l.alloc(32) == hipSuccess && g_live == 3);
    }
    CHECK(g_live == 0);
    printf("ok release: reset and scope end leave no live block\n");
}

static void move_transfers()
{
    Scratch<float> a;
    CHECK(a.alloc(4) == hipSuccess);
    float *pa = a.p;
    Scratch<float> b(std::move(a));
    CHECK(!a.p && b.p == pa && g_live == 1);
    Grown<int> g;
    CHECK(rzi::grow(drained, g.to(10)) == hipSuccess);
    int *pg = g;
    Grown<int> h(std::move(g));
    CHECK(!g && g.capacity() == 0 && h == pg && h.capacity() == 10);
    Grown<int> k;
    k = std::move(h);
    CHECK(!h && h.capacity() == 0 && k == pg && k.capacity() == 10 && g_live == 2);
    Lent<float> l;
    CHECK(l.alloc(4) == hipSuccess);
    float *pl = l;
    Lent<float> m(std::move(l));
    CHECK(!l && m == pl && g_live == 3);
    Lent<float> n;
    n = std::move(m);
    CHECK(!m && n == pl && g_live == 3);
    n = {};
    CHECK(g_live == 2);                 // the moved-to table owned it: resetting it frees
    printf("ok move: ownership transfers, the source is empty\n");
}

static void copy_borrows()
{
    const int frees0 = g_frees;
    {
        Lent<float> owner;
        CHECK(owner.alloc(8) == hipSuccess && g_live == 1);
        {
            Lent<float> alias(owner);
            CHECK(alias == owner && g_live == 1);
            Lent<float> assigned;
            assigned = owner;
            CHECK(assigned == owner);
            assigned = {};
            CHECK(!assigned && g_live == 1 && g_frees == frees0);      // resetting a copy frees nothing
        }
        CHECK(g_live == 1 && g_frees == frees0);                        // destroying the copies freed nothing
        static_cast<float *>(owner)[7] = 1.0f;                          // (ASan: the block is still there)
        // a struct of tables copies as a whole, as rz_fork copies RzStatic
        struct Table { Lent<float> a; Lent<int> b; unsigned n = 0; } t, fork;
        CHECK(t.a.alloc(4) == hipSuccess && t.b.alloc(4) == hipSuccess);
        t.n = 4;
        fork = t;
        CHECK(fork.a == t.a && fork.b == t.b && fork.n == 4 && g_live == 3);
        fork = {};
        CHECK(g_live == 3 && t.a && t.b);
        // a borrower that uploads its own table owns that one (it never happens in a fork: static_unlocked refuses)
        fork.a = t.a;
        CHECK(fork.a.alloc(4) == hipSuccess && fork.a != t.a && g_live == 4);
    }
    CHECK(g_live == 0 && g_frees == frees0 + 4);                        // each block freed once
    printf("ok copy: a copy of a static table aliases and frees nothing; the original frees once\n");
}

static void grow_cases()
{
    Grown<int> g;
    const int drains0 = g_drains;
    CHECK(rzi::grow(drained, g.to(4)) == hipSuccess && g.capacity() == 4 && g_drains == drains0 + 1);
    for (int i = 0; i < 4; ++i) g[i] = 10 + i;
    int *old = g;
    // a size that already fits: no allocation, no drain
    int allocs = g_allocs;
    CHECK(rzi::grow(drained, g.to(4)) == hipSuccess && rzi::grow(drained, g.to(1)) == hipSuccess);
    CHECK(g_allocs == allocs && g == old && g.capacity() == 4 && g_drains == drains0 + 1);
    // the replacement's allocation fails: pointer, capacity and contents stay, nothing drained
    g_fail_at = 1;
    CHECK(rzi::grow(drained, g.to(100)) == hipErrorOutOfMemory);
    CHECK(g == old && g.capacity() == 4 && g_live == 1 && g_drains == drains0 + 1);
    for (int i = 0; i < 4; ++i) CHECK(g[i] == 10 + i);
    // a drain that fails: the same
    CHECK(rzi::grow([] { return hipErrorUnknown; }, g.to(100)) == hipErrorUnknown);
    CHECK(g == old && g.capacity() == 4 && g_live == 1);
    for (int i = 0; i < 4; ++i) CHECK(g[i] == 10 + i);
    // success: the old block is freed exactly once
    int frees = g_frees;
    CHECK(rzi::grow(drained, g.to(100)) == hipSuccess);
    CHECK(g.capacity() == 100 && g_live == 1 && g_frees == frees + 1);
    g[99] = 1;
    // a set: the second member's allocation fails, every member stays; then all of them move together, none below its capacity
    Grown<int> a, b;
    Grown<float> w;
    CHECK(rzi::grow(drained, a.to(3), b.to(64), w.to(64 * 16)) == hipSuccess && g_live == 4);
    int *pa = a, *pb = b;
    float *pw = w;
    g_fail_at = 2;
    CHECK(rzi::grow(drained, a.to(9), b.to(65), w.to(65 * 16)) == hipErrorOutOfMemory);
    CHECK(a == pa && b == pb && w == pw && a.capacity() == 3 && b.capacity() == 64 && w.capacity() == 64 * 16 && g_live == 4);
    frees = g_frees;
    CHECK(rzi::grow(drained, a.to(2), b.to(65), w.to(65 * 16)) == hipSuccess);
    CHECK(a.capacity() == 3 && b.capacity() == 65 && w.capacity() == 65 * 16 && g_live == 4 && g_frees == frees + 3);
    a = {}; b = {}; w = {}; g = {};
    CHECK(g_live == 0);
    printf("ok grow: a failed grow keeps pointer, capacity and contents; a grow frees the old block once; a fit allocates nothing\n");
}

// the shape of rz_upload_ik: four arrays of one table filled one by one, the third allocation fails, the table is reset as a whole
static void partial_upload()
{
    struct Ik { Lent<int> chain, path, link, stage_off; unsigned n = 0; };
    auto upload = [](Ik &t) {
        if (t.chain.alloc(8) != hipSuccess) return false;
        if (t.path.alloc(8) != hipSuccess) return false;
        if (t.link.alloc(8) != hipSuccess) return false;
        if (t.stage_off.alloc(8) != hipSuccess) return false;
        t.n = 2;
        return true;
    };
    Ik resident;
    g_fail_at = 3;
    {
        Ik t;                           // the upload's local: a failure takes every array with it
        CHECK(!upload(t) && g_live == 2 && t.n == 0);
    }
    CHECK(g_live == 0);
    g_fail_at = 3;
    CHECK(!upload(resident) && g_live == 2);
    resident = {};
    CHECK(g_live == 0 && !resident.chain && !resident.path && resident.n == 0);
    CHECK(upload(resident) && g_live == 4);
    resident = {};
    CHECK(g_live == 0);
    printf("ok partial upload: a table reset as a whole strands nothing\n");
}

int main()
{
    release_by_reset_and_scope();
    move_transfers();
    copy_borrows();
    grow_cases();
    partial_upload();
    CHECK(g_live == 0 && g_allocs == g_frees);
    printf("ok all: %d blocks allocated, %d freed\n", g_allocs, g_frees);
    return 0;
}
