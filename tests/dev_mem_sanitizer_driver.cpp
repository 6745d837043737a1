// Driver of tests/test_dev_mem.py::test_owners_under_sanitizers: the owners of turbo_amd/csrc/dev_mem.hpp over a
// counting malloc policy that can fail the n-th allocation, the view and the synchronisation, compiled with
// -fsanitize=address,undefined.  A stand-alone program without any HIP header: CPU build only, never run on a GPU machine.
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "dev_mem.hpp"

static int g_checks = 0;
#define CHECK(x)                                                              \
    do {                                                                      \
        ++g_checks;                                                           \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); }  \
    } while (0)

struct Counting {
    using err_t = int;
    static constexpr int ok = 0;
    static int live, allocs, frees, fail_at, fail_view, ev_live, ev_made;   // fail_at: the n-th allocation from now fails (0: none)
    static int order[64], n_order;                                          // +1 allocation, -1 free, in the order they happened
    static int take(void **p, size_t bytes) {
        if (fail_at > 0 && --fail_at == 0) return 2;
        *p = malloc(bytes);
        ++live; ++allocs;
        if (n_order < 64) order[n_order++] = +1;
        return 0;
    }
    static void give(void *p) {
        free(p);
        --live; ++frees;
        if (n_order < 64) order[n_order++] = -1;
    }
    static int dev_alloc(void **p, size_t bytes) { return take(p, bytes); }
    static void dev_free(void *p) { give(p); }
    static int pin_alloc(void **h, size_t bytes, unsigned) { return take(h, bytes); }
    static int pin_view(void **d, void *h) {
        if (fail_view) return 3;
        *d = static_cast<char *>(h) + 1;   // (a view is another address of the same block)
        return 0;
    }
    static void pin_free(void *h) { give(h); }
    using event_t = int *;
    static int event_create(int **e, unsigned) { *e = new int(0); ++ev_live; ++ev_made; return 0; }
    static void event_destroy(int *e) { delete e; --ev_live; }
};
int Counting::live = 0, Counting::allocs = 0, Counting::frees = 0, Counting::fail_at = 0, Counting::fail_view = 0;
int Counting::ev_live = 0, Counting::ev_made = 0, Counting::order[64], Counting::n_order = 0;

template <class T> using Dev = tgp::DevBuf<T, Counting>;
template <class T> using Pin = tgp::PinBuf<T, Counting>;
using Ev = tgp::Event<Counting>;

static int g_syncs = 0;
static int sync_ok() { ++g_syncs; return 0; }
static int sync_bad() { ++g_syncs; return 7; }

// a group as tgp_internal.hpp's FitMem / WsMem: owners, an array of owners, generation defaults
struct Group {
    Dev<double> a, b;
    Dev<void> slab[2];
    Dev<char> never;          // stays empty
    long gen = -1;
    int S = 0;
    long ld = 0;
};

// the contract both buffer owners share; view(b): the device view when there is one, else the pointer again
template <class B, class View>
static void reserve_contract(B &b, View view) {
    const int a0 = Counting::allocs, f0 = Counting::frees, s0 = g_syncs;
    CHECK(b.get() == nullptr && b.bytes() == 0 && view(b) == nullptr);
    CHECK(b.reserve(0, sync_ok) == 0 && Counting::allocs == a0 && g_syncs == s0);       // nothing asked: nothing done
    CHECK(b.reserve(100, sync_ok) == 0 && b.get() && b.bytes() == 100 && view(b));
    CHECK(Counting::allocs == a0 + 1 && Counting::frees == f0 && g_syncs == s0 + 1);
    static_cast<char *>(static_cast<void *>(b.get()))[99] = 1;                           // (ASan: the block is that large)
    // smaller or equal: no allocation, no synchronisation, the same pointer
    auto *p = b.get();
    CHECK(b.reserve(100, sync_ok) == 0 && b.reserve(10, sync_ok) == 0 && b.reserve(10) == 0);
    CHECK(b.get() == p && b.bytes() == 100 && Counting::allocs == a0 + 1 && Counting::frees == f0 && g_syncs == s0 + 1);
    // larger: synchronise, free exactly once, then allocate
    Counting::n_order = 0;
    CHECK(b.reserve(300, sync_ok) == 0 && b.bytes() == 300 && b.get() && view(b));
    CHECK(Counting::allocs == a0 + 2 && Counting::frees == f0 + 1 && g_syncs == s0 + 2);
    CHECK(Counting::n_order == 2 && Counting::order[0] == -1 && Counting::order[1] == +1);
    static_cast<char *>(static_cast<void *>(b.get()))[299] = 1;
    // a failing synchronisation: pointer and size unchanged, nothing freed, nothing allocated
    p = b.get();
    CHECK(b.reserve(1000, sync_bad) == 7);
    CHECK(b.get() == p && b.bytes() == 300 && Counting::allocs == a0 + 2 && Counting::frees == f0 + 1);
    // a failing allocation: empty, the old block freed once; a later reserve succeeds
    Counting::fail_at = 1;
    CHECK(b.reserve(1000, sync_ok) == 2);
    CHECK(b.get() == nullptr && b.bytes() == 0 && view(b) == nullptr && !b);
    CHECK(Counting::allocs == a0 + 2 && Counting::frees == f0 + 2);
    CHECK(b.reserve(50, sync_ok) == 0 && b.get() && b.bytes() == 50 && view(b));
    CHECK(Counting::allocs == a0 + 3 && Counting::frees == f0 + 2);
    // reset, and reset again
    b.reset();
    CHECK(b.get() == nullptr && b.bytes() == 0 && view(b) == nullptr && Counting::frees == f0 + 3);
    b.reset();
    CHECK(Counting::frees == f0 + 3 && Counting::live == 0);
}

int main() {
    {   // the device buffer
        Dev<double> d;
        reserve_contract(d, [](const Dev<double> &b) { return b.get(); });
        CHECK(d.reserve(64) == 0);
        double *raw = d;                     // the implicit conversion the launchers rely on
        CHECK(raw == d.get() && d + 1 == raw + 1);
        Dev<void> v;
        CHECK(v.reserve(8) == 0 && static_cast<void *>(v) == v.get());
    }   // destruction frees both
    CHECK(Counting::live == 0);
    {   // the pinned buffer, mapped: host pointer and view are set and cleared together
        Pin<double> m(5u);
        reserve_contract(m, [](const Pin<double> &b) { return b.dev(); });
        CHECK(m.reserve(64, sync_ok) == 0 && m.dev() == reinterpret_cast<double *>(reinterpret_cast<char *>(m.get()) + 1));
        // the view fails after the allocation succeeded: the block goes back, both pointers stay null
        const int f0 = Counting::frees, a0 = Counting::allocs;
        Counting::fail_view = 1;
        CHECK(m.reserve(128, sync_ok) == 3);
        CHECK(m.get() == nullptr && m.dev() == nullptr && m.bytes() == 0 && Counting::frees == f0 + 2 && Counting::allocs == a0 + 1);
        Counting::fail_view = 0;
        CHECK(m.reserve(128, sync_ok) == 0 && m.get() && m.dev() && m.bytes() == 128);
        Pin<double> fresh(5u);
        m = std::move(fresh);                // move-assignment releases what it held
        CHECK(m.get() == nullptr && m.dev() == nullptr && m.bytes() == 0 && Counting::live == 0);
        CHECK(m.reserve(16) == 0);
        // unmapped: never a view
        Pin<unsigned> u(0u, false);
        Counting::fail_view = 1;             // (not even asked for)
        CHECK(u.reserve(40, sync_ok) == 0 && u.get() && u.dev() == nullptr && u.bytes() == 40);
        Counting::fail_view = 0;
    }
    CHECK(Counting::live == 0);
    {   // events
        Ev e;
        CHECK(static_cast<int *>(e) == nullptr && !e);
        CHECK(e.create(0) == 0 && e && Counting::ev_live == 1);
        int *h = e;
        CHECK(e.create(0) == 0 && static_cast<int *>(e) == h && Counting::ev_made == 1);   // exists: nothing happens
        std::vector<Ev> pool;
        for (int i = 0; i < 9; ++i) {        // (the vector moves them as it grows)
            Ev n;
            CHECK(n.create(2) == 0);
            pool.push_back(std::move(n));
        }
        CHECK(Counting::ev_live == 10 && pool[8]);
        pool[0] = Ev();                      // move-assignment destroys what it held
        CHECK(Counting::ev_live == 9 && !pool[0]);
        Ev arr[4];                           // empty owners can be destroyed
        (void)arr;
    }
    CHECK(Counting::ev_live == 0 && Counting::ev_made == 10);
    {   // a group: one assignment of a fresh struct releases it
        Group g;
        CHECK(g.a.reserve(80, sync_ok) == 0 && g.b.reserve(8) == 0 && g.slab[0].reserve(256) == 0 && g.slab[1].reserve(256) == 0);
        g.gen = 12; g.S = 5; g.ld = 768;
        CHECK(Counting::live == 4);
        const int f0 = Counting::frees, a0 = Counting::allocs;
        g = Group{};
        CHECK(Counting::frees == f0 + 4 && Counting::allocs == a0 && Counting::live == 0);   // each member exactly once
        CHECK(!g.a && !g.b && !g.slab[0] && !g.slab[1] && !g.never && g.a.bytes() == 0 && g.slab[1].bytes() == 0);
        CHECK(g.gen == -1 && g.S == 0 && g.ld == 0);
        // a set that fails half-way is released the same way, and the next attempt starts clean
        Counting::fail_at = 2;
        CHECK(g.a.reserve(80) == 0 && g.b.reserve(8) == 2 && Counting::live == 1);
        g = Group{};
        CHECK(Counting::live == 0 && g.a.reserve(80) == 0 && g.b.reserve(8) == 0 && Counting::live == 2);
        Group empty;                         // empty owners can be destroyed
        (void)empty;
    }   // destruction frees what the group holds
    CHECK(Counting::live == 0 && Counting::allocs == Counting::frees && Counting::ev_live == 0);
    printf("dev_mem ok: %d checks, %d allocations, %d frees\n", g_checks, Counting::allocs, Counting::frees);
    return 0;   // (ASan's leak check runs at exit)
}
