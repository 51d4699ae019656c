// The host code of epnn_coulomb_xyz_excl and epnn_coulomb_xyz_cell_excl that decides every index their kernel follows -- the list
// validator and CSR builder (excl_build) and the sizes of the two buffers the entries add -- run on the CPU over the shapes of
// tests/test_gpu_coulomb_excl.py and over every refusal.  No HIP call is made: build it for the host with the sanitizers and run it,
// from the repository root:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffinite-math-only -Xarch_host -fsanitize=address,undefined \
//           -Xarch_host -fno-sanitize-recover=undefined -o /tmp/excl_host_check tools/excl_host_check.hip -L/opt/rocm/lib -lrccl \
//           && /tmp/excl_host_check
// (the translation unit holds the kernels too, so the device pass runs, about a minute; the program needs no GPU)
#include "../epnn_amd/csrc/epnn_api.hip"

#include <cstdio>
#include <map>
#include <random>

static int fails = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

static bool says(const char *word) { return strstr(epnn_last_error(), word) != nullptr; }

// A list per molecule of n >= 2 atoms: a chain, atom 0 with up to 12 further partners, nothing on the last atom (n >= 3); shuffled,
// half of the rows swapped.  Then the CSR is checked against the list entry by entry.
static void check_batch(const std::vector<int> &ns, unsigned seed) {
    const int B = (int)ns.size();
    std::vector<int32_t> offsets(B + 1, 0);
    for (int b = 0; b < B; ++b) offsets[b + 1] = offsets[b] + ns[b];
    const int A = offsets[B];
    std::map<std::pair<int, int>, float> want;
    const float cycle[3] = {0.f, 0.5f, 0.8333f};
    int k = 0;
    for (int b = 0; b < B; ++b) {
        const int lo = offsets[b], top = ns[b] >= 3 ? ns[b] - 1 : ns[b];
        for (int a = 0; a + 1 < top; ++a) want[{lo + a, lo + a + 1}] = cycle[k++ % 3];
        for (int a = 2; a < top && a < 14; ++a) want[{lo, lo + a}] = 0.f;
    }
    std::vector<int32_t> ei, ej;
    std::vector<float> es;
    for (const auto &kv : want) { ei.push_back(kv.first.first); ej.push_back(kv.first.second); es.push_back(kv.second); }
    std::mt19937 rng(seed);
    const int64_t P = (int64_t)es.size();
    for (int64_t p = P - 1; p > 0; --p) {
        const int64_t o = (int64_t)(rng() % (unsigned)(p + 1));
        std::swap(ei[p], ei[o]); std::swap(ej[p], ej[o]); std::swap(es[p], es[o]);
    }
    for (int64_t p = 0; p < P; p += 2) std::swap(ei[p], ej[p]);
    ExclCsr ex;
    EXPECT(excl_build("check", B, offsets.data(), P, P ? ei.data() : nullptr, P ? ej.data() : nullptr, P ? es.data() : nullptr, ex) == 0);
    // buffer sizes: the scratch formula of include/epnn.h
    EXPECT(ex.blob.size() == ((size_t)A + 1) * 4 + 16 * (size_t)P && ex.blob.size() == excl_csr_bytes(A, P));
    EXPECT(ex.o_partner() == ((size_t)A + 1) * 4 && ex.o_factor() == ex.o_partner() + 8 * (size_t)P && ex.o_factor() + 8 * (size_t)P == ex.blob.size());
    EXPECT(excl_xpart_bytes(A, false) == (size_t)A * 32 && excl_xpart_bytes(A, true) == (size_t)A * 80);
    EXPECT(excl_xpart_bytes(A, true) == (size_t)A * EW_PART * 8 && excl_xpart_bytes(A, false) == (size_t)A * CL_XPART * 8);
    const int *row_off = ex.row_off(), *partner = ex.partner();
    const float *factor = ex.factor();
    EXPECT(ex.A == A && ex.P == P && row_off[0] == 0 && (int64_t)row_off[A] == 2 * P);
    std::map<std::pair<int, int>, int> seen;
    for (int b = 0; b < B; ++b)
        for (int a = offsets[b]; a < offsets[b + 1]; ++a) {
            EXPECT(row_off[a] <= row_off[a + 1]);
            for (int e = row_off[a]; e < row_off[a + 1]; ++e) {
                const int j = partner[e];
                EXPECT(j >= offsets[b] && j < offsets[b + 1] && j != a);                    // inside the atom's own molecule
                EXPECT(e == row_off[a] || partner[e - 1] < j);                             // sorted, no partner twice
                const auto key = std::make_pair(std::min(a, j), std::max(a, j));
                EXPECT(want.count(key) == 1 && factor[e] == want[key] - 1.f);
                ++seen[key];
            }
        }
    EXPECT(seen.size() == want.size());
    for (const auto &kv : seen) EXPECT(kv.second == 2);                                   // every pair exactly twice
    // the same CSR whatever the order of the list and of a pair's two atoms
    std::vector<int32_t> si, sj;
    std::vector<float> ss;
    for (const auto &kv : want) { si.push_back(kv.first.first); sj.push_back(kv.first.second); ss.push_back(kv.second); }
    ExclCsr sorted;
    EXPECT(excl_build("check", B, offsets.data(), P, si.data(), sj.data(), ss.data(), sorted) == 0);
    EXPECT(sorted.blob == ex.blob);
}

int main() {
    for (int n : {1, 2, 3, 17, 63, 64, 65, 129, 257}) check_batch({n}, 100u + (unsigned)n);
    check_batch({20, 1, 9, 30}, 7u);
    check_batch({70, 1, 33, 120, 300, 2, 1}, 8u);
    // ---- refusals, each by name and with the pair's position; a good list afterwards
    const int32_t offsets[4] = {0, 5, 6, 10};
    const int32_t gi[4] = {0, 1, 6, 9}, gj[4] = {1, 4, 7, 8};
    const float gs[4] = {0.f, 0.5f, 1.f, 0.8333f};
    ExclCsr ex;
    // (the factor comes as its bits: this program is built with -ffinite-math-only too, where an infinity may not be named as a float)
    auto with_bits = [&](int64_t P, int at, int32_t i, int32_t j, uint32_t sbits) {
        int32_t vi[4], vj[4];
        float vs[4];
        for (int k = 0; k < 4; ++k) { vi[k] = k == at ? i : gi[k]; vj[k] = k == at ? j : gj[k]; vs[k] = gs[k]; }
        if (at >= 0) memcpy(&vs[at], &sbits, 4);
        return excl_build("check", 3, offsets, P, vi, vj, vs, ex);
    };
    auto with = [&](int64_t P, int at, int32_t i, int32_t j, float s) {
        uint32_t bits;
        memcpy(&bits, &s, 4);
        return with_bits(P, at, i, j, bits);
    };
    EXPECT(with(4, -1, 0, 0, 0.f) == 0);
    EXPECT(with(-1, -1, 0, 0, 0.f) == 1 && says("negative"));
    EXPECT(excl_build("check", 3, offsets, (int64_t)1 << 30, gi, gj, gs, ex) == 1 && says("2^31 - 1"));
    EXPECT(excl_build("check", 3, offsets, 4, nullptr, gj, gs, ex) == 1 && says("NULL"));
    EXPECT(excl_build("check", 3, offsets, 4, gi, nullptr, gs, ex) == 1 && says("NULL"));
    EXPECT(excl_build("check", 3, offsets, 4, gi, gj, nullptr, ex) == 1 && says("NULL"));
    EXPECT(excl_build("check", 3, offsets, 0, nullptr, nullptr, nullptr, ex) == 0 && ex.blob.size() == 11 * 4 && ex.row_off()[10] == 0);
    EXPECT(with(4, 2, 10, 7, 0.f) == 1 && says("pair 2") && says("outside [0, 10)"));
    EXPECT(with(4, 3, 7, -1, 0.f) == 1 && says("pair 3") && says("outside"));
    EXPECT(with(4, 1, 3, 3, 0.f) == 1 && says("pair 1") && says("itself"));
    EXPECT(with(4, 1, 4, 5, 0.f) == 1 && says("pair 1") && says("different molecules"));
    EXPECT(with(4, 0, 4, 6, 0.f) == 1 && says("pair 0") && says("different molecules"));
    EXPECT(with(4, 3, 1, 0, 0.5f) == 1 && says("pair 3") && says("listed twice") && says("pair 0"));
    EXPECT(with(4, 2, 1, 4, 0.5f) == 1 && says("listed twice"));
    EXPECT(with_bits(4, 2, 6, 7, 0x7f800000u) == 1 && says("pair 2") && says("not finite"));
    EXPECT(with_bits(4, 0, 0, 1, 0x7fc00000u) == 1 && says("pair 0") && says("not finite"));
    EXPECT(with_bits(4, 0, 0, 1, 0xff800000u) == 1 && says("not finite"));
    EXPECT(with(4, -1, 0, 0, 0.f) == 0 && ex.row_off()[10] == 8);
    printf(fails ? "%d checks failed\n" : "exclusion host checks passed\n", fails);
    return fails ? 1 : 0;
}
