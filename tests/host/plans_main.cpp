// The plan registry of a handle (dl-unet_amd/csrc/plans.hpp) on the CPU, with an int as the payload: a stand-alone program
// that tests/test_plans_cpu.py compiles with the host compiler (address and undefined-behaviour sanitizers where the
// compiler has them) and runs.  Prints one line per case and "plans OK"; the exit status is the number of failed checks.
#include "../../dl-unet_amd/csrc/plans.hpp"

#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

using Reg = unet::PlanRegistry<int>;

static int failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { ++failures; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// keys are addresses the registry never dereferences: 256-byte steps like workspaces
static const void *key(size_t i) { return (const void *)(uintptr_t)(0x10000 + 256 * i); }

static bool has(const Reg &r, size_t i, int want)
{
    int v = -1;
    return r.lookup(key(i), v) && v == want;
}
static bool absent(const Reg &r, size_t i)
{
    int v = -12345;
    return !r.lookup(key(i), v) && v == -12345;      // a failed lookup leaves the caller's value alone
}

static void replacement_at_the_same_address()
{
    Reg r;
    r.remember(key(0), 1);
    r.remember(key(1), 2);
    r.remember(key(0), 3);
    CHECK(r.size() == 2 && has(r, 0, 3) && has(r, 1, 2) && r.pending(key(0)));
    // a finished entry that is planned again is pending again, and holds no place among the finished ones
    CHECK(r.finish(key(0)) && !r.pending(key(0)));
    r.remember(key(0), 4);
    CHECK(r.size() == 2 && has(r, 0, 4) && r.pending(key(0)) && r.pending_count() == 2);
    std::printf("replacement at the same address\n");
}

static void one_pending_entry_survives_finished_ones(size_t n)
{
    Reg r;
    r.remember(key(0), 77);
    for (size_t i = 1; i <= n; ++i) {
        r.remember(key(i), (int)i);
        CHECK(r.finish(key(i)));
    }
    CHECK(has(r, 0, 77) && r.pending(key(0)) && r.pending_count() == 1);
    CHECK(r.size() == 1 + (n < Reg::FINISHED_KEPT ? n : Reg::FINISHED_KEPT));
    // the same with the finished steps all on ONE other address (a training loop that reuses its workspace)
    Reg q;
    q.remember(key(0), 77);
    for (size_t i = 1; i <= n; ++i) { q.remember(key(1), (int)i); q.finish(key(1)); }
    CHECK(has(q, 0, 77) && has(q, 1, (int)n) && q.size() == 2);
    std::printf("one pending entry survives %zu finished ones\n", n);
}

static void many_pending_at_once()
{
    Reg r;
    for (size_t i = 0; i < 17; ++i) r.remember(key(i), (int)i);
    for (size_t i = 0; i < 17; ++i) CHECK(has(r, i, (int)i));
    // up to the documented bound every pending entry is kept; one more drops the oldest pending one
    for (size_t i = 17; i < Reg::PENDING_MAX; ++i) r.remember(key(i), (int)i);
    CHECK(r.pending_count() == Reg::PENDING_MAX && has(r, 0, 0));
    r.remember(key(Reg::PENDING_MAX), -1);
    CHECK(r.pending_count() == Reg::PENDING_MAX && absent(r, 0) && has(r, 1, 1) && has(r, Reg::PENDING_MAX, -1));
    CHECK(Reg::PENDING_MAX >= 1024);
    std::printf("17 and PENDING_MAX pending at once\n");
}

static void finished_entries_leave_oldest_first()
{
    Reg r;
    const size_t K = Reg::FINISHED_KEPT;
    for (size_t i = 0; i < K + 4; ++i) r.remember(key(i), (int)i);
    // finished in another order than planned: the age is that of the finish, so the one just finished never leaves
    for (size_t i = K + 4; i-- > 0;) {
        r.finish(key(i));
        CHECK(has(r, i, (int)i) && !r.pending(key(i)));
        CHECK(r.size() == K + 4 - (K + 4 - i > K ? K + 4 - i - K : 0));
    }
    for (size_t i = K; i < K + 4; ++i) CHECK(absent(r, i));
    for (size_t i = 0; i < K; ++i) CHECK(has(r, i, (int)i) && !r.pending(key(i)));
    // the oldest forward finishes last, after K others: it stays readable and the first finished leaves
    Reg d;
    d.remember(key(0), 100);
    for (size_t i = 1; i <= K; ++i) { d.remember(key(i), (int)i); d.finish(key(i)); }
    CHECK(d.finish(key(0)) && has(d, 0, 100) && absent(d, 1) && has(d, 2, 2) && d.size() == K);
    // exactly K finished entries are not too many: none leaves before the (K+1)-th
    Reg q;
    for (size_t i = 0; i < K; ++i) { q.remember(key(i), (int)i); q.finish(key(i)); }
    CHECK(q.size() == K && has(q, 0, 0));
    q.remember(key(K), (int)K);
    CHECK(q.size() == K + 1 && has(q, 0, 0));        // a pending one pushes nothing out
    q.finish(key(K));
    CHECK(q.size() == K && absent(q, 0) && has(q, 1, 1));
    q.finish(key(K));                                // finishing twice changes nothing
    CHECK(q.size() == K && has(q, 1, 1));
    std::printf("finished entries leave oldest first\n");
}

static void forget_and_unknown_addresses()
{
    Reg r;
    CHECK(absent(r, 0) && !r.forget(key(0)) && !r.finish(key(0)) && !r.pending(key(0)) && r.size() == 0);
    CHECK(absent(r, 0) && r.size() == 0);            // none of those created an entry
    r.remember(key(0), 5);
    r.remember(key(2), 6);
    CHECK(absent(r, 1));                             // between two known addresses
    int v = 0;
    CHECK(!r.lookup((const char *)key(0) + 1, v) && !r.lookup(nullptr, v));
    CHECK(r.forget(key(0)) && absent(r, 0) && has(r, 2, 6) && r.size() == 1);
    CHECK(!r.forget(key(0)));
    r.finish(key(2));
    CHECK(r.forget(key(2)) && r.size() == 0);
    r.remember(key(0), 9);                           // a forgotten address can be planned again
    CHECK(has(r, 0, 9) && r.pending(key(0)));
    std::printf("forget, and addresses never inserted\n");
}

static void four_threads_on_disjoint_addresses()
{
    Reg r;
    const size_t T = 4, N = 200;
    std::vector<int> bad(T, 0);
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t)
        th.emplace_back([&r, &bad, t] {
            for (size_t round = 0; round < 3; ++round)
                for (size_t i = 0; i < N; ++i) {
                    const size_t k = t * N + i;
                    r.remember(key(k), (int)(k + round));
                    int v = -1;
                    if (!r.lookup(key(k), v) || v != (int)(k + round)) ++bad[t];
                    if (i > 0 && (!r.lookup(key(k - 1), v) || v != (int)(k - 1 + round))) ++bad[t];
                }
        });
    for (std::thread &x : th) x.join();
    for (size_t t = 0; t < T; ++t) CHECK(bad[t] == 0);
    CHECK(r.size() == T * N && r.pending_count() == T * N);
    for (size_t k = 0; k < T * N; ++k) CHECK(has(r, k, (int)(k + 2)));
    std::printf("four threads, disjoint addresses\n");
}

int main()
{
    replacement_at_the_same_address();
    one_pending_entry_survives_finished_ones(16);
    one_pending_entry_survives_finished_ones(17);
    one_pending_entry_survives_finished_ones(1000);
    many_pending_at_once();
    finished_entries_leave_oldest_first();
    forget_and_unknown_addresses();
    four_threads_on_disjoint_addresses();
    if (failures == 0) std::printf("plans OK\n");
    return failures > 100 ? 100 : failures;
}
