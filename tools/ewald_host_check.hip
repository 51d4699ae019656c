// The host code of epnn_coulomb_xyz_cell that decides every loop bound of its kernels -- the parameter rule (epnn_ewald_params), the
// check of an `ewald` row (ew_cell_row) and the task builders (cl_build_tasks, ew_build_tasks) -- run on the CPU over the shapes of
// tests/test_gpu_coulomb_cell.py, with every task checked against the arrays it indexes.  No HIP call is made: build it for the host
// with the sanitizers and run it, from the repository root:
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffinite-math-only -Xarch_host -fsanitize=address,undefined \
//           -Xarch_host -fno-sanitize-recover=undefined -o /tmp/ewald_host_check tools/ewald_host_check.hip -L/opt/rocm/lib -lrccl \
//           && /tmp/ewald_host_check
// (the translation unit holds the kernels too, so the device pass runs, about a minute; the program needs no GPU)
#include "../epnn_amd/csrc/epnn_api.hip"

#include <cstdio>

static int fails = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

static void check_batch(const std::vector<int> &ns, const std::vector<const float *> &cells, double alpha, double tol) {
    const int B = (int)ns.size();
    std::vector<int32_t> offsets(B + 1, 0);
    for (int b = 0; b < B; ++b) offsets[b + 1] = offsets[b] + ns[b];
    const int A = offsets[B];
    std::vector<EwCell> ew(B);
    for (int b = 0; b < B; ++b) {
        double row[6];
        EXPECT(epnn_ewald_params(cells[b], alpha, tol, row) == 0);
        EXPECT(ew_cell_row("check", b, cells[b], row, alpha, ew[b]) == 0);
        EXPECT(ew[b].ns == (2 * ew[b].M0 + 1) * (2 * ew[b].M1 + 1) * (ew[b].M2 + 1) && ew[b].ns >= 1 && ew[b].ns <= EW_SLOT_CAP);
        // the slot of m = 0, which k_ew_atom and k_ew_energy read, lies in the box
        EXPECT(ew[b].M1 * (2 * ew[b].M0 + 1) + ew[b].M0 < ew[b].ns);
    }
    std::vector<int4> ctasks, atasks;
    std::vector<int2> stasks;
    const int cpieces = cl_build_tasks(B, offsets.data(), ctasks);
    const size_t slots = ew_build_tasks(B, offsets.data(), ew, atasks, stasks);
    std::vector<int> seen((size_t)A * (size_t)cpieces, 0), aseen(A, 0);
    for (const int4 &t : ctasks) {
        const int na = t.y & 255, piece = t.y >> 8;
        EXPECT(na >= 1 && na <= CL_BLOCK && t.x >= 0 && t.x + na <= A && piece >= 0 && piece < cpieces);
        EXPECT(t.z >= 0 && t.z <= t.w && t.w <= A);
        for (int l = 0; l < na; ++l) ++seen[(size_t)piece * A + t.x + l];
    }
    for (int b = 0; b < B; ++b)
        for (int a = offsets[b]; a < offsets[b + 1]; ++a)
            for (int k = 0; k < cl_pieces(ns[b]); ++k) EXPECT(seen[(size_t)k * A + a] == 1);       // written by exactly one wavefront
    for (const int4 &t : atasks) {
        EXPECT(t.y >= 1 && t.y <= EW_TILE && t.z >= 0 && t.z < B && t.x >= offsets[t.z] && t.x + t.y <= offsets[t.z + 1] && t.w == ns[t.z]);
        for (int l = 0; l < t.y; ++l) ++aseen[t.x + l];
    }
    for (int a = 0; a < A; ++a) EXPECT(aseen[a] == 1);
    std::vector<char> sseen(slots, 0);
    for (const int2 &t : stasks) {
        EXPECT(t.x >= 0 && t.x < B && t.y >= 0 && t.y < ew[t.x].ns && t.y % EW_TILE == 0);
        for (int l = 0; l < EW_TILE && t.y + l < ew[t.x].ns; ++l) ++sseen[(size_t)ew[t.x].soff + t.y + l];
    }
    for (size_t s = 0; s < slots; ++s) EXPECT(sseen[s] == 1);
}

int main() {
    const float cube8[9] = {8, 0, 0, 0, 8, 0, 0, 0, 8}, sheared[9] = {7, 0, 0, 1.5f, 6.5f, 0, -1, 2, 8}, slab[9] = {6, 0, 0, 0, 6, 0, 0, 0, 20},
                cube14[9] = {14, 0, 0, 0, 14, 0, 0, 0, 14}, open_z[9] = {8, 0, 0, 0, 8, 0, 0, 0, 0}, needle[9] = {6, 0, 0, 0, 6, 0, 0, 0, 20000};
    for (double alpha : {0.0, 0.5, 0.05})
        for (double tol : {1e-6, 1e-8}) {
            for (const float *cell : {cube8, sheared, slab, cube14})
                for (int n : {1, 2, 17, 63, 64, 65, 128, 129, 257}) check_batch({n}, {cell}, alpha, tol);
            check_batch({20, 1, 9, 30}, {cube8, sheared, slab, cube14}, alpha, tol);
            check_batch({70, 1, 33, 120, 300}, {cube8, sheared, slab, cube14, cube14}, alpha, tol);
        }
    double row[6];
    EwCell e;
    EXPECT(epnn_ewald_params(open_z, 0.0, 1e-6, row) == 1);
    EXPECT(epnn_ewald_params(needle, 0.0, 1e-6, row) == 1);
    EXPECT(epnn_ewald_params(cube8, 0.0, 0.0, row) == 1 && epnn_ewald_params(cube8, 0.0, 1.0, row) == 1);
    EXPECT(epnn_ewald_params(cube8, -1.0, 1e-6, row) == 1 && epnn_ewald_params(nullptr, 0.0, 1e-6, row) == 1);
    EXPECT(epnn_ewald_params(cube8, 0.0, 1e-6, row) == 0 && ew_cell_row("check", 0, cube8, row, 0.0, e) == 0);
    const double good[6] = {row[0], row[1], row[2], row[3], row[4], row[5]};
    auto with = [&](int k, double v) { double r[6]; for (int i = 0; i < 6; ++i) r[i] = i == k ? v : good[i]; return ew_cell_row("check", 0, cube8, r, 0.0, e); };
    EXPECT(with(1, 4.0001) == 1 && with(1, 4.0) == 0 && with(1, -1.0) == 1 && with(1, 0.0) == 1);
    EXPECT(with(0, 0.0) == 1 && with(0, -1.0) == 1 && with(2, -1.0) == 1);
    EXPECT(with(3, good[3] - 1.0) == 1 && with(4, 2.5) == 1 && with(5, 1e9) == 1 && with(5, 5000.0) == 1 && with(5, good[5] + 3.0) == 0);
    printf(fails ? "%d checks failed\n" : "ewald host checks passed\n", fails);
    return fails ? 1 : 0;
}
