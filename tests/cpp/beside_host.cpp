// csrc/host/beside.h without a device and without libmi_dspu.so: the five mi_dspu_* functions that the header calls are defined
// here over host memory (every block exactly as large as asked for, so that the address sanitizer sees a write past
// rows * cap floats), with a switch that makes the next allocation fail and a count of the live ones.  One line per check;
// tests/test_beside_host.py builds this with -fsanitize=address,undefined and holds the lines to what they must say.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>

#include "beside.h"

namespace
{
    std::atomic<int> g_live(0), g_mallocs(0);
    size_t g_last_bytes = 0;
    bool g_fail_next = false;
}

extern "C"
{
int mi_dspu_malloc(void **dev_ptr, size_t bytes)
{
    if (g_fail_next)
    {
        g_fail_next = false;
        return MI_OK - 1;
    }
    *dev_ptr = malloc(bytes);
    ++g_live, ++g_mallocs;
    g_last_bytes = bytes;
    return MI_OK;
}

int mi_dspu_free(void *dev_ptr)
{
    if (dev_ptr != nullptr)
        --g_live;
    free(dev_ptr);
    return MI_OK;
}

int mi_dspu_copy_h2d(void *dev_dst, const void *host_src, size_t bytes, void *) { memcpy(dev_dst, host_src, bytes); return MI_OK; }
int mi_dspu_copy_d2h(void *host_dst, const void *dev_src, size_t bytes, void *) { memcpy(host_dst, dev_src, bytes); return MI_OK; }
int mi_dspu_stream_synchronize(void *) { return MI_OK; }
}

namespace
{
    using mi_host::rows;

    static_assert(!std::is_copy_constructible<rows>::value && !std::is_copy_assignable<rows>::value, "rows is not copied");

    void rows_reserve()
    {
        rows r;
        const int before = g_mallocs;
        const size_t asks[5][2] = { { 4, 2 }, { 3, 2 }, { 4, 1 }, { 5, 2 }, { 4, 3 } };
        printf("reserve");
        for (size_t i = 0; i < 5; ++i)
        {
            const bool ok = r.reserve(asks[i][0], asks[i][1]);
            printf(" %d %d %zu %zu %zu", ok ? 1 : 0, int(g_mallocs) - before, r.capacity(), r.nrows(), g_last_bytes);
        }
        printf("\n");
        printf("row %td %td %td\n", r.row(0) - r.row(0), r.row(1) - r.row(0), r.row(2) - r.row(0));
    }

    // every row up and down again with n floats; the rows next to it keep what they held
    bool round_trip(rows &r, size_t n)
    {
        const size_t cap = r.capacity(), k = r.nrows();
        std::vector<float> all(k * cap, -1.0f), back(cap);
        mi_dspu_copy_h2d(r.row(0), all.data(), k * cap * sizeof(float), nullptr);
        bool ok = true;
        for (size_t row = 0; row < k; ++row)
        {
            std::vector<float> src(n);
            for (size_t i = 0; i < n; ++i)
                src[i] = float(100 * row + i);
            ok = ok && r.up(row, src.data(), n) && r.down(back.data(), row, n) && memcmp(back.data(), src.data(), n * sizeof(float)) == 0;
        }
        mi_dspu_copy_d2h(all.data(), r.row(0), k * cap * sizeof(float), nullptr);
        for (size_t row = 0; row < k; ++row)
            for (size_t i = 0; i < cap; ++i)
                ok = ok && all[row * cap + i] == ((i < n) ? float(100 * row + i) : -1.0f);
        return ok;
    }

    void rows_copies()
    {
        rows r;
        r.reserve(7, 3);
        printf("roundtrip %d %d\n", round_trip(r, 1) ? 1 : 0, round_trip(r, r.capacity()) ? 1 : 0);
    }

    void rows_failure_and_destructor()
    {
        const int before = g_live;
        {
            rows r;
            r.reserve(4, 2);
            const int held = g_live - before;
            g_fail_next = true;
            const bool failed = r.reserve(8, 2);
            printf("failed %d %d %zu %zu %d", held, failed ? 1 : 0, r.capacity(), r.nrows(), int(g_live) - before);
            const bool again = r.reserve(8, 2);
            printf(" %d %zu %zu %d\n", again ? 1 : 0, r.capacity(), r.nrows(), int(g_live) - before);
        }
        printf("destroyed %d\n", int(g_live) - before);
        rows never;
        never.release();
        printf("empty %d %zu %d\n", never.row(0) == nullptr ? 1 : 0, never.capacity(), int(g_live) - before);
    }

    // an entry that counts itself and owns rows, as the wrappers' entries do
    struct fake
    {
        static std::atomic<int> made, gone;
        int tag = 0;
        rows buf;
        fake()  { ++made; }
        ~fake() { ++gone; }
    };
    std::atomic<int> fake::made(0), fake::gone(0);
    typedef mi_host::registry<fake> fakes;

    int g_makes = 0;
    int make_ok(fake &e)    { e.tag = ++g_makes; return e.buf.reserve(16, 2) ? MI_OK : MI_OK - 1; }
    int make_bad(fake &e)   { ++g_makes; e.buf.reserve(16, 2); return MI_OK - 1; }

    void registry_cases()
    {
        int here[4];
        const int live = g_live;
        fake *a = fakes::of(&here[0], make_ok), *b = fakes::of(&here[0], make_ok);
        printf("of_twice %d %d %d %d\n", (a != nullptr && a == b) ? 1 : 0, g_makes, int(fake::made), int(fake::gone));

        fake *c = fakes::of(&here[1], make_bad);
        printf("make_fails %d %d %d %d %d", c == nullptr ? 1 : 0, fakes::find(&here[1]) == nullptr ? 1 : 0, g_makes, int(fake::made), int(fake::gone));
        c = fakes::of(&here[1], make_ok);
        printf(" %d %d %d %d\n", c != nullptr ? 1 : 0, g_makes, int(fake::made), int(fake::gone));

        fakes::drop(&here[0]);
        printf("drop %d %d", int(fake::gone), fakes::find(&here[0]) == nullptr ? 1 : 0);
        fakes::drop(&here[0]);
        fakes::drop(&here[2]);                                  // never known
        printf(" %d %d\n", int(fake::gone), int(fake::made));

        fake *d = fakes::of(&here[0], make_ok);
        printf("again %d %d %d\n", d != nullptr ? d->tag : 0, g_makes, int(fake::made));

        const int made = fake::made;
        printf("find %d %d %d\n", fakes::find(&here[3]) == nullptr ? 1 : 0, fakes::find(&here[0]) == d ? 1 : 0, int(fake::made) - made);

        fakes::drop(&here[0]);
        fakes::drop(&here[1]);
        printf("balance %d %d %d\n", int(fake::made), int(fake::gone), int(g_live) - live);
    }

    void registry_threads()
    {
        static char where[4][64];
        const int made = fake::made, gone = fake::gone, live = g_live;
        std::atomic<int> wrong(0);
        std::vector<std::thread> pool;
        for (int t = 0; t < 4; ++t)
            pool.emplace_back([t, &wrong]()
            {
                for (int i = 0; i < 64; ++i)
                {
                    fake *p = fakes::of(&where[t][i], [](fake &e) { return e.buf.reserve(8, 1) ? MI_OK : MI_OK - 1; });
                    if (p == nullptr || fakes::find(&where[t][i]) != p)
                        ++wrong;
                }
                for (int i = 0; i < 64; ++i)
                    fakes::drop(&where[t][i]);
            });
        for (std::thread &th : pool)
            th.join();
        int left = 0;
        for (int t = 0; t < 4; ++t)
            for (int i = 0; i < 64; ++i)
                left += (fakes::find(&where[t][i]) != nullptr) ? 1 : 0;
        printf("threads %d %d %d %d %d\n", int(wrong), left, int(fake::made) - made, int(fake::gone) - gone, int(g_live) - live);
    }

    // beside<>: the entry's destructor destroys the bank that make created, and none where make failed
    struct bank_t { int channels; };
    int g_banks = 0, g_destroyed = 0;
    int bank_create(bank_t **b, uint32_t channels)  { *b = new bank_t{ int(channels) }; ++g_banks; return MI_OK; }
    int bank_refuse(bank_t **, uint32_t)            { return MI_OK - 1; }
    int bank_destroy(bank_t *b)                     { delete b; ++g_destroyed; return MI_OK; }
    struct held_t { uint32_t word = 0; };
    typedef mi_host::registry<mi_host::beside<bank_t, held_t, bank_destroy> > banks;

    void beside_cases()
    {
        int here[2];
        const int live = g_live;
        banks::entry *p = banks::of_one(&here[0], bank_create);
        int sent = 0;
        const auto send = [&sent](bank_t *, const held_t &) { ++sent; return int(MI_OK); };
        held_t now;
        const bool same = p->hand_over_state(now, send);
        now.word = 7;
        const bool other = p->hand_over_state(now, send) && p->hand_over_state(now, send);
        p->buf.reserve(5, 3);
        printf("beside %d %d %d %d %d %u", p->bank->channels, same ? 1 : 0, other ? 1 : 0, sent, int(g_live) - live, p->held.word);
        banks::drop(&here[0]);
        printf(" %d %d %d", g_banks, g_destroyed, int(g_live) - live);
        printf(" %d %d\n", banks::of_one(&here[1], bank_refuse) == nullptr ? 1 : 0, g_destroyed);
    }
}

int main()
{
    rows_reserve();
    rows_copies();
    rows_failure_and_destructor();
    registry_cases();
    registry_threads();
    beside_cases();
    printf("live %d\n", int(g_live));
    return 0;
}
