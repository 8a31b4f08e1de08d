// stage_main.cpp — the staging layout of rbp_session_refill_from_plans (csrc/common/plan_stage.h) checked on the host, stand-alone:
// tests/test_plan_stage.py builds this with g++ -fsanitize=address,undefined and runs it.
//
// For N = 1, 4, 5 agents and slot strides 27 and 65 it packs five missions of ragged M out of {2, 3, 20, 26} with block sizes that give
// one round, rounds of one mission, and rounds of two with a short last round; walks every round's flat index space with the header's
// element rules into an arena image that starts out as garbage; and requires that the image equals one built directly (compact rows,
// zero tails), that every destination element of the slots 0 .. K-1 was written exactly once, and that nothing else was written.  The
// round's tables are compared with their sources as mission_gather_element (kernels/handoff.hip) indexes them.  Last it prints the packer's
// total for capacity-shaped missions, which the Python test compares with rbp_plan_stage_bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common/plan_stage.h"

namespace ps = plan_stage;

#define REQUIRE(cond, ...)                                  \
    do {                                                    \
        if (!(cond)) {                                      \
            std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
            std::exit(1);                                   \
        }                                                   \
    } while (0)

struct Mission {
    int M, MB;
    unsigned long long world[ps::WORLD_WORDS];
    std::vector<double> T, start, goal, radius, max_vel, max_acc;
    std::vector<float> traj;
};

static unsigned rng_state = 12345u;
static double next_value() {  // never zero: a zero tail is then told from data
    rng_state = rng_state * 1664525u + 1013904223u;
    return 1.0 + (rng_state >> 8) / 16777216.0;
}

static Mission make_mission(int N, int M, int id) {
    Mission m;
    m.M = M, m.MB = M - 1 + id % 2;
    for (int w = 0; w < ps::WORLD_WORDS; ++w) m.world[w] = 0x1000ull * (id + 1) + w;
    auto fill = [](std::vector<double>& v, size_t n) {
        v.resize(n);
        for (double& x : v) x = next_value();
    };
    fill(m.T, M + 1), fill(m.start, 9 * N), fill(m.goal, 9 * N), fill(m.radius, N), fill(m.max_vel, 3 * N), fill(m.max_acc, 3 * N);
    m.traj.resize((size_t)3 * N * (M + 1));
    for (float& x : m.traj) x = (float)next_value();
    return m;
}

// one partition: packs and walks round after round; returns the number of rounds
static int run_case(int N, int stride, const std::vector<Mission>& ms, size_t block_bytes, const std::vector<int>& expect_rounds) {
    const int K = (int)ms.size(), slots = K + 1;  // one slot beyond the batch, which nothing may touch
    const long long slot_f = 3LL * N * stride;
    const float junk_f = -7.5f;
    const double junk_d = -9.25;
    std::vector<float> traj((size_t)slot_f * slots, junk_f), want_traj = traj;
    std::vector<double> T((size_t)stride * slots, junk_d), want_T = T;
    std::vector<int> n_traj(traj.size(), 0), n_T(T.size(), 0);
    for (int j = 0; j < K; ++j) {  // the image built directly: a compact copy at the front of the slot, zeros behind it
        for (long long f = 0; f < slot_f; ++f) want_traj[j * slot_f + f] = f < (long long)ms[j].traj.size() ? ms[j].traj[f] : 0.0f;
        for (int t = 0; t < stride; ++t) want_T[(size_t)j * stride + t] = t <= ms[j].M ? ms[j].T[t] : 0.0;
    }
    std::vector<int> Mk(K);
    for (int j = 0; j < K; ++j) Mk[j] = ms[j].M;
    // the block is exactly block_bytes long, so that the sanitizer sees a round that runs over it
    std::vector<int> rounds;
    for (int j0 = 0; j0 < K;) {
        const int j1 = ps::round_end(Mk.data(), K, N, j0, block_bytes), n = j1 - j0;
        REQUIRE(j1 > j0, "mission %d does not fit %zu bytes", j0, block_bytes);
        REQUIRE(j1 == K || ps::round_bytes(Mk.data(), N, j0, j1 + 1) > block_bytes, "round [%d, %d) is not greedy", j0, j1);
        char* block = static_cast<char*>(std::malloc(block_bytes));
        std::memset(block, 0xAB, block_bytes);
        std::vector<ps::Source> src(n);
        for (int r = 0; r < n; ++r) {
            const Mission& m = ms[j0 + r];
            src[r] = ps::Source{m.M, m.MB, m.world, m.T.data(), m.traj.data(), m.start.data(), m.goal.data(), m.radius.data(), m.max_vel.data(), m.max_acc.data()};
        }
        const size_t bytes = ps::pack_round(block, src.data(), n, N);
        REQUIRE(bytes == ps::round_bytes(Mk.data(), N, j0, j1) && bytes <= block_bytes, "round [%d, %d): %zu bytes packed", j0, j1, bytes);
        const ps::Round R{j0, n, N, stride};
        for (long long i = 0; i < ps::traj_elements(R); ++i) {
            long long dst = -1;
            const float v = ps::traj_element(block, R, i, &dst);
            REQUIRE(dst >= 0 && dst < (long long)traj.size(), "init_traj index %lld", dst);
            traj[dst] = v, ++n_traj[dst];
        }
        for (long long i = 0; i < ps::time_elements(R); ++i) {
            long long dst = -1;
            const double v = ps::time_element(block, R, i, &dst);
            REQUIRE(dst >= 0 && dst < (long long)T.size(), "T index %lld", dst);
            T[dst] = v, ++n_T[dst];
        }
        // the tables: entries, the source list, and the five arrays read as [src[r] * N ...]
        const int* ids = reinterpret_cast<const int*>(block + ps::off_src(n));
        auto dbl = [&](size_t off) { return reinterpret_cast<const double*>(block + off); };
        for (int r = 0; r < n; ++r) {
            const Mission& m = ms[j0 + r];
            const ps::Entry& e = ps::entry(block, r);
            REQUIRE(e.Mk == m.M && e.MBk == m.MB && !std::memcmp(e.world, m.world, sizeof(m.world)), "entry %d of round at %d", r, j0);
            REQUIRE(e.off_T % 8 == 0 && e.off_traj % 4 == 0 && e.off_traj + 4 * m.traj.size() <= bytes, "offsets of entry %d", r);
            REQUIRE(ids[r] == r, "source list");
            const size_t s = (size_t)ids[r] * N;
            REQUIRE(!std::memcmp(dbl(ps::off_start(n)) + 9 * s, m.start.data(), 72 * N), "start %d", r);
            REQUIRE(!std::memcmp(dbl(ps::off_goal(n, N)) + 9 * s, m.goal.data(), 72 * N), "goal %d", r);
            REQUIRE(!std::memcmp(dbl(ps::off_radius(n, N)) + s, m.radius.data(), 8 * N), "radius %d", r);
            REQUIRE(!std::memcmp(dbl(ps::off_max_vel(n, N)) + 3 * s, m.max_vel.data(), 24 * N), "max_vel %d", r);
            REQUIRE(!std::memcmp(dbl(ps::off_max_acc(n, N)) + 3 * s, m.max_acc.data(), 24 * N), "max_acc %d", r);
        }
        std::free(block);
        rounds.push_back(n);
        j0 = j1;
    }
    REQUIRE(rounds == expect_rounds, "N = %d stride = %d block = %zu: %zu rounds", N, stride, block_bytes, rounds.size());
    REQUIRE(!std::memcmp(traj.data(), want_traj.data(), sizeof(float) * traj.size()), "init_traj image, N = %d stride = %d", N, stride);
    REQUIRE(!std::memcmp(T.data(), want_T.data(), sizeof(double) * T.size()), "T image, N = %d stride = %d", N, stride);
    for (size_t i = 0; i < traj.size(); ++i) REQUIRE(n_traj[i] == (i < (size_t)slot_f * K ? 1 : 0), "init_traj element %zu written %d times", i, n_traj[i]);
    for (size_t i = 0; i < T.size(); ++i) REQUIRE(n_T[i] == (i < (size_t)stride * K ? 1 : 0), "T element %zu written %d times", i, n_T[i]);
    return (int)rounds.size();
}

int main() {
    const int Ms[5] = {20, 2, 26, 3, 26};
    int cases = 0;
    for (int N : {1, 4, 5})
        for (int stride : {27, 65}) {
            std::vector<Mission> ms;
            std::vector<int> Mk;
            for (int j = 0; j < 5; ++j) ms.push_back(make_mission(N, Ms[j], j)), Mk.push_back(Ms[j]);
            const size_t all = ps::round_bytes(Mk.data(), N, 0, 5);
            const size_t one = ps::mission_bytes(N, 26);                             // the largest mission alone
            const size_t two = ps::mission_bytes(N, 26) + ps::mission_bytes(N, 3);   // the larger of the pairs (20, 2) and (26, 3)
            run_case(N, stride, ms, all, {5});
            run_case(N, stride, ms, all + 1000, {5});
            run_case(N, stride, ms, one, {1, 1, 1, 1, 1});
            run_case(N, stride, ms, two, {2, 2, 1});
            cases += 4;
        }
    // capacity-shaped missions: what rbp_plan_stage_bytes must answer
    for (int N : {1, 4, 64})
        for (int M : {2, 26, 64})
            for (int K : {1, 2, 7}) {
                std::vector<Mission> ms;
                std::vector<ps::Source> src;
                for (int j = 0; j < K; ++j) ms.push_back(make_mission(N, M, j));
                for (const Mission& m : ms)
                    src.push_back(ps::Source{m.M, m.MB, m.world, m.T.data(), m.traj.data(), m.start.data(), m.goal.data(), m.radius.data(), m.max_vel.data(), m.max_acc.data()});
                std::vector<char> block(ps::mission_bytes(N, M) * K);
                std::printf("capacity %d %d %d %zu\n", N, M, K, ps::pack_round(block.data(), src.data(), K, N));
            }
    std::printf("ok %d cases\n", cases);
    return 0;
}
