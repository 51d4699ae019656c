// The host code of epnn_coulomb_xyz_cell and epnn_coulomb_xyz_slab that decides every loop bound of their kernels -- the parameter rules
// (epnn_ewald_params, epnn_ewald_slab_params), the check of an `ewald` row (ew_row_check through ew_cell_row and sl_cell_row), the
// slab's slot list, the task builders (cl_build_tasks, ew_build_tasks) and the driver's byte layout (coulomb_layout) -- run on the CPU
// over the shapes of tests/test_gpu_coulomb_cell.py and tests/test_gpu_coulomb_slab.py, with every task checked against the arrays it
// indexes and every layout against the formulas of include/epnn.h; and the site entries' argument checks and per-atom rows (site_build,
// site_width_check) on arrays of exactly the stated lengths, the slab case of the width check and the slab kind of the layout
// (epnn_coulomb_xyz_slab_site) included.  No HIP call is made: build it for the host
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

// the sweeps' task table (all six entries): every (piece, atom) row is written by exactly one wavefront
static std::vector<int32_t> check_ctasks(const std::vector<int> &ns) {
    const int B = (int)ns.size();
    std::vector<int32_t> offsets(B + 1, 0);
    for (int b = 0; b < B; ++b) offsets[b + 1] = offsets[b] + ns[b];
    const int A = offsets[B];
    std::vector<int4> ctasks;
    const int cpieces = cl_build_tasks(B, offsets.data(), ctasks);
    std::vector<int> seen((size_t)A * (size_t)cpieces, 0);
    for (const int4 &t : ctasks) {
        const int na = t.y & 255, piece = t.y >> 8;
        EXPECT(na >= 1 && na <= CL_BLOCK && t.x >= 0 && t.x + na <= A && piece >= 0 && piece < cpieces);
        EXPECT(t.z >= 0 && t.z <= t.w && t.w <= A);
        for (int l = 0; l < na; ++l) ++seen[(size_t)piece * A + t.x + l];
    }
    for (int b = 0; b < B; ++b)
        for (int a = offsets[b]; a < offsets[b + 1]; ++a)
            for (int k = 0; k < cl_pieces(ns[b]); ++k) EXPECT(seen[(size_t)k * A + a] == 1);
    return offsets;
}

static void check_batch(const std::vector<int> &ns, const std::vector<const float *> &cells, double alpha, double tol) {
    const int B = (int)ns.size();
    const std::vector<int32_t> offsets = check_ctasks(ns);
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
    std::vector<int4> atasks;
    std::vector<int2> stasks;
    const size_t slots = ew_build_tasks(B, offsets.data(), ew, atasks, stasks);
    std::vector<int> aseen(A, 0);
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

// A slab batch: the rule, then the row's check, must pass; every cell's slots are the half plane inside kc, once each, behind the batch's
static void check_slab_batch(const std::vector<int> &ns, const std::vector<const float *> &cells, double alpha, double tol) {
    const int B = (int)cells.size();
    check_ctasks(ns);                                            // (the slab's two sweeps run on this table alone)
    std::vector<EwCell> ew(B);
    std::vector<SlCell> sl(B);
    std::vector<SlSlot> slots;
    for (int b = 0; b < B; ++b) {
        double row[6];
        SlGeom G;
        const size_t before = slots.size();
        EXPECT(epnn_ewald_slab_params(cells[b], alpha, tol, row) == 0);
        EXPECT(sl_cell_geom("check", b, cells[b], G) == 0 && row[3 + G.open] == 0.0);
        EXPECT(sl_cell_row("check", b, cells[b], row, alpha, ew[b], sl[b], slots) == 0);
        EXPECT((size_t)sl[b].soff == before && (size_t)sl[b].ns == slots.size() - before && sl[b].ns <= SL_SLOT_CAP);
        EXPECT((ew[b].rc == 0.f) == (row[1] == 0.0) && (double)ew[b].rc <= row[1] && ew[b].beta == (float)row[0]);
        const double Ma = row[3 + G.pa], Mb = row[3 + G.pb];
        std::vector<char> seen((size_t)((2 * Ma + 1) * (Mb + 1)), 0);
        for (size_t k = before; k < slots.size(); ++k) {
            const SlSlot &t = slots[k];
            EXPECT(t.m1 > 0.0 || (t.m1 == 0.0 && t.m0 > 0.0));
            EXPECT(fabs(t.m0) <= Ma && t.m1 <= Mb && t.k > 0.0 && t.k <= row[2] && t.u == 0.5 * t.k / row[0]);
            for (float v : {t.w, t.wk, t.kx, t.ky, t.kz, t.ik}) EXPECT(epnn_finite(v));
            EXPECT(epnn_finite(t.k) && epnn_finite(t.u) && t.m0 == floor(t.m0) && t.m1 == floor(t.m1));
            if (!(fabs(t.m0) <= Ma && t.m1 >= 0.0 && t.m1 <= Mb)) continue;
            EXPECT(seen[(size_t)(t.m1 * (2 * Ma + 1) + t.m0 + Ma)]++ == 0);        // no (m0, m1) twice
        }
    }
}

// coulomb_layout against the byte formulas the two drivers it replaced computed by hand, for one batch of each kind
static void check_layouts() {
    const size_t A = 459, B = 3, nct = 21, nat = 9, nst = 37, cp = 3, slots = 5819;        // (nst odd: the stasks end off a multiple of 16)
    auto r16 = [](size_t v) { return (v + 15) & ~size_t(15); };
    const size_t o_E = (((A * 4 + 1) * 4) + 7) & ~size_t(7);
    CoulombLayout L = coulomb_layout(CL_OPEN, false, A, B, nct, 0, 0, cp, 0);
    EXPECT(L.blob_bytes == nct * 16 && L.E == o_E && L.gsf == o_E + B * 8 && L.co_bytes == L.gsf);
    EXPECT(L.part_bytes == cp * A * 4 * 8 && L.share == L.part_bytes && L.sc_bytes == L.share + A * 8);
    L = coulomb_layout(CL_CELL, true, A, B, nct, nat, nst, cp, slots);
    EXPECT(L.atasks == nct * 16 && L.stasks == L.atasks + nat * 16 && L.ew == L.stasks + r16(nst * 8) && L.blob_bytes == L.ew + B * sizeof(EwCell));
    EXPECT(L.E == o_E && L.gsf == o_E + B * 8 && L.co_bytes == L.gsf + B * 36);
    EXPECT(L.part_bytes == cp * A * EW_PART * 8 && L.share == L.part_bytes && L.S == r16(L.share + A * EW_SHARE * 8) && L.rec == L.S + slots * 16 &&
           L.sc_bytes == L.rec + slots * 16);
    for (bool strain : {false, true}) {
        L = coulomb_layout(CL_SLAB, strain, A, B, nct, 0, 0, cp, slots);
        EXPECT(L.ew == nct * 16 && L.sl == L.ew + r16(B * sizeof(EwCell)) && L.slot == L.sl + B * sizeof(SlCell) &&
               L.blob_bytes == L.slot + slots * sizeof(SlSlot));
        EXPECT(L.E == o_E && L.gsf == o_E + B * 8 && L.co_bytes == L.gsf + (strain ? B * 36 : 0));
        EXPECT(L.part_bytes == cp * A * EW_PART * 8 && L.rpart == L.part_bytes && L.share == L.rpart + cp * A * (strain ? SL_PART_STRAIN : SL_PART) * 8);
        EXPECT(L.sc_bytes == L.share + A * 8 + (strain ? A * SL_SHARE_W * 8 : 0) && (!strain || L.wshare == L.share + A * 8));
    }
}

// The site entries' host part: site_build reads exactly A values of each array it is given (the arrays here are heap blocks of exactly
// that length: a read past them is the sanitizer's to report) and writes A rows, each the float64 formula rounded once; every
// refusal of include/epnn.h; the cells' width check at and around its limit; the layout's added segments.
static void check_site() {
    const std::vector<int> ns = {70, 1, 33, 120};
    const int B = (int)ns.size();
    std::vector<int32_t> offsets(B + 1, 0);
    for (int b = 0; b < B; ++b) offsets[b + 1] = offsets[b] + ns[b];
    const int A = offsets[B];
    std::vector<float> sigma(A), chi(A), hard(A);
    for (int a = 0; a < A; ++a) {
        sigma[a] = 0.3f + 0.9f * (float)((a * 37) % 101) / 100.f;
        chi[a] = (float)((a * 17) % 23) / 7.f - 1.5f;
        hard[a] = 2.f + (float)((a * 5) % 13);
    }
    for (int self_term : {0, 1})
        for (int mask = 0; mask < 8; ++mask) {
            const float *sg = mask & 1 ? sigma.data() : nullptr, *ch = mask & 2 ? chi.data() : nullptr, *hd = mask & 4 ? hard.data() : nullptr;
            for (double alpha : {0.0, 0.7}) {
                CoulombSite site;
                const int rc = site_build("check", B, offsets.data(), alpha, sg, ch, hd, self_term, site);
                const bool refused = (sg && alpha > 0.0) || (self_term && !sg && !(alpha > 0.0));
                EXPECT(rc == (refused ? 1 : 0));
                if (rc) continue;
                EXPECT((int)site.rows.size() == A && (int)site.sigma_max.size() == B && site.widths == (sg != nullptr));
                for (int b = 0; b < B; ++b) {
                    double top = 0.0;
                    for (int a = offsets[b]; a < offsets[b + 1]; ++a) {
                        const float4 r = site.rows[a];
                        const double s = (double)sigma[a];
                        EXPECT(r.x == (sg ? (float)(2.0 * s * s) : 0.f) && r.y == (ch ? chi[a] : 0.f) && r.z == (hd ? hard[a] : 0.f));
                        EXPECT(r.w == (self_term ? (float)(sg ? 0.5 / s : alpha) : 0.f));
                        EXPECT(epnn_finite(r.x) && epnn_finite(r.w) && (!sg || r.x > 0.f));
                        top = std::max(top, s);
                    }
                    EXPECT(site.sigma_max[b] == (sg ? top : 0.0));
                }
            }
        }
    CoulombSite sink;
    auto with = [&](std::vector<float> &v, int k, float bad, const float *sg, const float *ch, const float *hd) {
        const float keep = v[k];
        v[k] = bad;
        const int rc = site_build("check", B, offsets.data(), 0.0, sg, ch, hd, 0, sink);
        v[k] = keep;
        return rc;
    };
    // (infinities and a NaN come as their bits: this program is built with -ffinite-math-only, where they may not be named as floats)
    auto bits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
    const float inf = bits(0x7f800000u), minf = bits(0xff800000u), nan = bits(0x7fc00000u);
    for (float bad : {0.f, -0.5f, inf, minf, nan, 1e-30f, 1e25f}) EXPECT(with(sigma, A - 1, bad, sigma.data(), nullptr, nullptr) == 1);
    EXPECT(with(sigma, 0, 1e-19f, sigma.data(), nullptr, nullptr) == 0 && with(sigma, 0, 1e18f, sigma.data(), nullptr, nullptr) == 0);
    for (float bad : {inf, minf, nan}) {
        EXPECT(with(chi, 7, bad, sigma.data(), chi.data(), hard.data()) == 1 && with(hard, A - 1, bad, nullptr, chi.data(), hard.data()) == 1);
        EXPECT(with(chi, 7, bad, sigma.data(), nullptr, hard.data()) == 0);                // (an array that is not given is not read)
    }
    EXPECT(site_build("check", B, offsets.data(), 0.0, sigma.data(), nullptr, nullptr, 2, sink) == 1);
    EXPECT(site_build("check", B, offsets.data(), 0.0, sigma.data(), nullptr, nullptr, -1, sink) == 1);
    // the width check: gamma_min = 1 / (2 sigma_max) >= beta
    EXPECT(site_width_check("check", 0, 0.5, 1.0) == 0 && site_width_check("check", 0, 0.5000001, 1.0) == 1 && site_width_check("check", 0, 0.0, 1.0) == 0);
    EXPECT(site_width_check("check", 2, 1.2, 0.3) == 0 && site_width_check("check", 2, 1.2, 0.42) == 1);
    // the layout: mu behind the strain rows, the per-cell sums behind rec, the rows' span; nothing else moves
    const size_t nct = 21, nat = 9, nst = 37, cp = 3, slots = 5819;
    for (CoulombKind kind : {CL_OPEN, CL_CELL, CL_SLAB})
        for (bool strain : {false, true}) {
            if (strain != (kind == CL_CELL) && kind != CL_SLAB) continue;            // (open: never, cells: always, slabs: both entries)
            const CoulombLayout P = coulomb_layout(kind, strain, (size_t)A, (size_t)B, nct, nat, nst, cp, slots),
                                S = coulomb_layout(kind, strain, (size_t)A, (size_t)B, nct, nat, nst, cp, slots, true);
            EXPECT(P.site_bytes == 0 && P.mu == 0 && P.wsum == 0 && S.site_bytes == (size_t)A * 16);
            EXPECT(S.blob_bytes == P.blob_bytes && S.E == P.E && S.gsf == P.gsf && S.mu == P.co_bytes && S.co_bytes == P.co_bytes + (size_t)A * 4);
            EXPECT(S.part_bytes == P.part_bytes && S.share == P.share && S.S == P.S && S.rec == P.rec);
            EXPECT(S.rpart == P.rpart && S.wshare == P.wshare && S.ew == P.ew && S.sl == P.sl && S.slot == P.slot);
            // slabs have no per-cell sum: the sweeps' buffer does not grow
            EXPECT(kind != CL_CELL ? (S.sc_bytes == P.sc_bytes && S.wsum == 0)
                                   : (S.wsum == P.sc_bytes && S.sc_bytes == P.sc_bytes + (size_t)B * 8 && S.wsum % 8 == 0));
        }
}

// The slab case of the width check (epnn_coulomb_xyz_slab_site): at the beta of the slab rule, tol = 1e-6 and alpha = 0, a cell's widest
// Gaussian passes at 1 / (2 beta) and is refused just above it, in the words of the periodic entry: the cell, sigma_max and the limit.
static void check_slab_width(const std::vector<const float *> &cells) {
    const char *name = "epnn_coulomb_xyz_slab_site";
    for (int b = 0; b < (int)cells.size(); ++b) {
        double row[6];
        EXPECT(epnn_ewald_slab_params(cells[b], 0.0, 1e-6, row) == 0 && row[1] > 0.0);
        const double limit = 0.5 / row[0];
        EXPECT(site_width_check(name, b, limit, row[0]) == 0 && site_width_check(name, b, 0.4 * limit, row[0]) == 0);
        EXPECT(site_width_check(name, b, 0.0, row[0]) == 0);                           // (no widths given: sigma_max is 0)
        EXPECT(site_width_check(name, b, limit * (1.0 + 1e-9), row[0]) == 1);
        char want[256];
        snprintf(want, sizeof(want), "%s: cell %d: sigma_max = %g is above the largest width 1 / (2 beta) = %g ", name, b, limit * (1.0 + 1e-9), limit);
        EXPECT(strncmp(epnn_last_error(), want, strlen(want)) == 0);
    }
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
    // ---- slabs: the cells and sizes of tests/test_gpu_coulomb_slab.py (the rule and the slots depend on the cell alone)
    const float sq65[9] = {6.5f, 0, 0, 0, 6.5f, 0, 0, 0, 0}, sl_sheared[9] = {7, 0, 0, 2, 6.9f, 0, 0, 0, 0}, tilted[9] = {0, 0, 0, 6.8f, 1.0f, 1.5f, -0.5f, 6.0f, 3.5f},
                openy[9] = {7, 0, 0, 0, 0, 0, 2, 0, 6.9f}, sq14[9] = {14, 0, 0, 0, 14, 0, 0, 0, 0};
    for (double alpha : {0.0, 0.5, 0.05})
        for (double tol : {1e-6, 1e-8}) {
            for (const float *cell : {sq65, sl_sheared, tilted, openy, sq14})
                for (int n : {1, 2, 17, 63, 64, 65, 128, 129, 257}) check_slab_batch({n}, {cell}, alpha, tol);
            check_slab_batch({20, 1, 9, 30}, {sq65, tilted, openy, sq14}, alpha, tol);
            check_slab_batch({70, 1, 33, 120, 300}, {sq65, sl_sheared, tilted, openy, sq14}, alpha, tol);
        }
    check_layouts();
    check_site();
    check_slab_width({sq65, sl_sheared, tilted, openy, sq14});
    // the shared row check through the slab path
    SlGeom G;
    SlCell c;
    std::vector<SlSlot> sink;
    EXPECT(epnn_ewald_slab_params(openy, 0.0, 1e-6, row) == 0 && sl_cell_geom("check", 0, openy, G) == 0 && G.open == 1 && G.pa == 0 && G.pb == 2);
    const double sgood[6] = {row[0], row[1], row[2], row[3], row[4], row[5]};
    auto swith = [&](int k, double v, double alpha = 0.0) {
        double r[6];
        for (int i = 0; i < 6; ++i) r[i] = i == k ? v : sgood[i];
        return sl_cell_row("check", 0, openy, r, alpha, e, c, sink);
    };
    EXPECT(swith(1, sgood[1]) == 0 && sgood[1] == 0.5 * G.wmin && swith(1, sgood[1] * (1 + 1e-12)) == 1 && swith(1, -1.0) == 1);
    EXPECT(swith(1, 0.0) == 1 && swith(1, 0.0, 2.0) == 1 && swith(1, 0.0, sgood[0]) == 0);       // rc = 0 takes beta == alpha > 0
    EXPECT(swith(4, 1.0) == 1 && swith(3, 2.5) == 1 && swith(5, sgood[5] - 1.0) == 1 && swith(3, sgood[3] - 1.0) == 1 && swith(5, sgood[5] + 2.0) == 0);
    EXPECT(swith(0, 0.0) == 1 && swith(2, -1.0) == 1);
    const float wire[9] = {7, 0, 0, 0, 0, 0, 0, 0, 0}, parallel[9] = {7, 0, 0, 14, 0, 0, 0, 0, 0};
    for (const float *bad : {cube8, wire, parallel}) {
        EXPECT(epnn_ewald_slab_params(bad, 0.0, 1e-6, row) == 1);
        EXPECT(sl_cell_row("check", 0, bad, sgood, 0.0, e, c, sink) == 1);
    }
    printf(fails ? "%d checks failed\n" : "ewald host checks passed\n", fails);
    return fails ? 1 : 0;
}
