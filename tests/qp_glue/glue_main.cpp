// The order of operations of the batch QP's workgroup-wide reductions (csrc/common/reduce_order.h) as g++ compiles it, restated lane by
// lane (tests/test_qp_glue.py builds this program with the sanitizers and runs it).
//
//   1. the tree is a reduction: in every step a lane combines with a lane whose partial result covers OTHER lanes of the row, after the
//      four steps every lane of a row covers its 16 lanes exactly once, partner() is an involution inside the row;
//   2. K values reduced together (block_reduce_n: the steps interleaved over the values, the wavefronts' results parked in chunks of the
//      16 scratch slots) give, per value, the bits of K separate reductions (block_reduce) -- for K = 1 .. 4, sum / max / min mixed, 256
//      and 512 threads; no slot is written twice or read unwritten inside a chunk, none lies outside the scratch;
//   3. the data can tell: the same values summed in another order -- lane after lane, or with two steps of the tree exchanged -- give
//      another last bit.
// Both models of 2 walk the same header, so what 2 really checks is the slot / chunk map (interleaving independent chains cannot change a
// value on the host).  The DEVICE code is not covered here: it is held to the parent commit's bits by the benchmark's dumped outputs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common/reduce_order.h"

using namespace red_order;

static int failures = 0;
#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            if (failures < 20) std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond);   \
            ++failures;                                                                            \
        }                                                                                          \
    } while (0)

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
static double red_op(double a, double b, int op) { return op == 0 ? a + b : (op == 1 ? std::fmax(a, b) : std::fmin(a, b)); }

// one step of the tree on a wavefront: every lane combines with its partner's value of BEFORE the step
static void row_step(double* v, int step, int op) {
    double in[64];
    std::memcpy(in, v, sizeof in);
    for (int l = 0; l < 64; ++l) v[l] = red_op(in[l], in[partner(step, l)], op);
}
static double rows_combine(const double* v, int op) { return red_op(red_op(v[0], v[16], op), red_op(v[32], v[48], op), op); }

// block_reduce: one value, its own pair of barriers
static double reduce_one(const std::vector<double>& x, int op, const int* step_order = nullptr) {
    const int waves = (int)x.size() / 64;
    double r = 0;
    for (int w = 0; w < waves; ++w) {
        double v[64];
        std::memcpy(v, &x[64 * w], sizeof v);
        for (int s = 0; s < ROW_STEPS; ++s) row_step(v, step_order ? step_order[s] : s, op);
        const double wr = rows_combine(v, op);
        r = w == 0 ? wr : red_op(r, wr, op);
    }
    return r;
}

// block_reduce_n: K values, steps interleaved, the wavefronts' results through the scratch in chunks
static void reduce_n(const std::vector<std::vector<double>>& x, const std::vector<int>& op, std::vector<double>& out) {
    const int K = (int)x.size(), waves = (int)x[0].size() / 64, CH = chunk(waves);
    CHECK(CH >= 1);
    std::vector<std::vector<double>> v(x);           // [K][threads]
    for (int s = 0; s < ROW_STEPS; ++s)              // (interleaved: step s of every value before step s + 1 of any)
        for (int q = 0; q < K; ++q)
            for (int w = 0; w < waves; ++w) row_step(&v[q][64 * w], s, op[q]);
    std::vector<std::vector<double>> wr(K, std::vector<double>(waves));
    for (int q = 0; q < K; ++q)
        for (int w = 0; w < waves; ++w) wr[q][w] = rows_combine(&v[q][64 * w], op[q]);
    out.assign(K, 0.0);
    for (int q0 = 0; q0 < K; q0 += CH) {
        double red[SLOTS];
        bool written[SLOTS] = {};
        for (int w = 0; w < waves; ++w)              // lane 0 of every wavefront
            for (int q = q0; q < K && q < q0 + CH; ++q) {
                const int sl = slot(q - q0, w, waves);
                CHECK(sl >= 0 && sl < SLOTS);
                if (sl < 0 || sl >= SLOTS) continue;
                CHECK(!written[sl]);
                written[sl] = true, red[sl] = wr[q][w];
            }
        // (barrier)
        for (int q = q0; q < K && q < q0 + CH; ++q) {
            double r = 0;
            for (int i = 0; i < waves; ++i) {
                const int sl = slot(q - q0, i, waves);
                CHECK(sl >= 0 && sl < SLOTS && written[sl]);
                if (sl < 0 || sl >= SLOTS) continue;
                r = i == 0 ? red[sl] : red_op(r, red[sl], op[q]);
            }
            out[q] = r;
        }
        // (barrier)
    }
}

static void the_tree_is_a_reduction() {
    for (int s = 0; s < ROW_STEPS; ++s)
        for (int l = 0; l < 64; ++l) {
            const int p = partner(s, l);
            CHECK(p >= 0 && p < 64 && p / 16 == l / 16 && p != l && partner(s, p) == l);
        }
    uint64_t cover[64];
    for (int l = 0; l < 64; ++l) cover[l] = 1ull << l;
    for (int s = 0; s < ROW_STEPS; ++s) {
        uint64_t in[64];
        std::memcpy(in, cover, sizeof in);
        for (int l = 0; l < 64; ++l) {
            CHECK((in[l] & in[partner(s, l)]) == 0);   // nothing is counted twice
            cover[l] = in[l] | in[partner(s, l)];
        }
    }
    for (int l = 0; l < 64; ++l) CHECK(cover[l] == 0xffffull << (16 * (l / 16)));
    CHECK(DPP_CTRL[0] == 0xB1 && DPP_CTRL[1] == 0x4E && DPP_CTRL[2] == 0x141 && DPP_CTRL[3] == 0x140);
    CHECK(chunk(4) == 4 && chunk(8) == 2);
}

// values whose sum rounds in (nearly) every addition: magnitudes over twelve binades, both signs, from a fixed-seed generator
static std::vector<double> draw(int n, uint64_t seed) {
    std::vector<double> x(n);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    for (int i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const double m = 1.0 + (double)(s >> 11) * 0x1p-53;            // [1, 2): 53 significant bits
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const int e = (int)((s >> 33) % 12) - 6;
        x[i] = std::ldexp(((s >> 60) & 1) ? -m : m, e);
    }
    return x;
}

static void together_is_separate() {
    int told_lanewise = 0, told_swapped = 0, sums = 0;
    for (int threads : {256, 512})
        for (int K = 1; K <= 4; ++K)
            for (int trial = 0; trial < 8; ++trial) {
                std::vector<std::vector<double>> x;
                std::vector<int> op;
                for (int q = 0; q < K; ++q) x.push_back(draw(threads, 1000u * threads + 100u * K + 10u * trial + q)), op.push_back((q + trial) % 3);
                std::vector<double> got;
                reduce_n(x, op, got);
                for (int q = 0; q < K; ++q) {
                    const double want = reduce_one(x[q], op[q]);
                    CHECK(bits(got[q]) == bits(want));
                    if (op[q] != 0) continue;
                    ++sums;
                    double lanewise = 0;
                    for (double t : x[q]) lanewise += t;
                    const int swapped[ROW_STEPS] = {3, 1, 2, 0};
                    told_lanewise += bits(lanewise) != bits(want);
                    told_swapped += bits(reduce_one(x[q], 0, swapped)) != bits(want);
                }
            }
    std::printf("sums %d: another last bit lane after lane %d, with steps 0 and 3 exchanged %d\n", sums, told_lanewise, told_swapped);
    // (an order that happens to round alike on one draw is possible; on most of them it must not)
    CHECK(sums >= 40 && 2 * told_lanewise > sums && 2 * told_swapped > sums);
    // the kernel's uses: (gap, pres), (dmax, gmax), (gap_next, pres_next, pmin), (vmax, q0, q1, q2)
    const std::vector<std::vector<int>> uses = {{0, 1}, {1, 1}, {0, 1, 2}, {1, 0, 0, 0}};
    for (int threads : {256, 512})
        for (const auto& op : uses) {
            std::vector<std::vector<double>> x;
            for (size_t q = 0; q < op.size(); ++q) x.push_back(draw(threads, 77u + threads + q));
            std::vector<double> got;
            reduce_n(x, op, got);
            for (size_t q = 0; q < op.size(); ++q) CHECK(bits(got[q]) == bits(reduce_one(x[q], op[q])));
        }
}

int main() {
    the_tree_is_a_reduction();
    together_is_separate();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("qp glue ok\n");
    return 0;
}
