// bsk_config.hip — the configuration arithmetic of the C-ABI: bsk_default_config, the checks of a bsk_config and everything the
// kernels read that is derived from one on the host (StepParams / ColdCfg, the two spherical-harmonics coefficient streams).
// Pure arithmetic: this unit calls no HIP runtime function and defines no kernel.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "bsk_capi.hpp"

namespace bsk { namespace capi __attribute__((visibility("hidden"))) {

bool inv3(const double* m, double* o) {
    double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    if (!(std::fabs(det) > 0.0)) return false;
    double id = 1.0 / det;
    o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
    return true;
}

// Low-precision solar position (Astronomical Almanac), equatorial frame, metres, Earth-centred.
// Stands in for the SPICE de430 lookup at reference leoPowerAttitudeSimulator.py:219-225.
void sun_position(double jd, double out[3]) {
    const double D2R = M_PI / 180.0, AU = 149597870700.0;
    double n = jd - 2451545.0;
    double L = std::fmod(280.460 + 0.9856474 * n, 360.0), g = std::fmod(357.528 + 0.9856003 * n, 360.0) * D2R;
    double lam = (L + 1.915 * std::sin(g) + 0.020 * std::sin(2 * g)) * D2R;
    double eps = (23.439 - 0.0000004 * n) * D2R;
    double R = (1.00014 - 0.01671 * std::cos(g) - 0.00014 * std::cos(2 * g)) * AU;
    out[0] = R * std::cos(lam);
    out[1] = R * std::cos(eps) * std::sin(lam);
    out[2] = R * std::sin(eps) * std::sin(lam);
}

// Fused Pines coefficient stream for gravity_sh (bsk_device.hpp), iteration order
// M = 1..d+1, L = M..d+1, 8 doubles per step:
//   [0] L == M: A[M][M] (diagonal constant);  L == M+1: A[M+1][M]/(u A[M][M]);  else n1[L][M]
//   [1] n2[L][M] (L >= M+2)                      -- recursion A[L][M] = u n1 A[L-1][M] - n2 A[L-2][M]
//   [2,3] M (Cbar, Sbar)[L][M]                   -- a1 / a2 sums            (L <= d)
//   [4,5] nq1[L][M-1] (Cbar, Sbar)[L][M-1]       -- a3 sum                  (L <= d)
//   [6,7] nq2[L-1][M-1] (Cbar, Sbar)[L-1][M-1]   -- a4 sum                  (L >= 2)
// Constants as Basilisk's gravityEffector documents them (SURVEY.md §8 note N1).
void build_sh_table(int d, const double* cbar, const double* sbar, std::vector<double>& tab) {
    auto K = [](int i) { return i == 0 ? 1.0 : 2.0; };
    auto idx = [](int l, int m) { return l * (l + 1) / 2 + m; };
    std::vector<double> diag(d + 2), sd(d + 2);
    diag[0] = 1.0;
    for (int l = 1; l <= d + 1; ++l) diag[l] = std::sqrt((double)(2 * l + 1) * K(l) / ((double)(2 * l) * K(l - 1))) * diag[l - 1];
    for (int l = 1; l <= d + 1; ++l) sd[l] = std::sqrt((double)(2 * l) * K(l - 1) / K(l)) * diag[l];
    auto n1 = [](int l, int m) { return std::sqrt((double)(2 * l + 1) * (double)(2 * l - 1) / ((double)(l - m) * (double)(l + m))); };
    auto n2 = [](int l, int m) {
        return std::sqrt((double)(l + m - 1) * (double)(2 * l + 1) * (double)(l - m - 1) /
                         ((double)(l + m) * (double)(l - m) * (double)(2 * l - 3)));
    };
    auto nq1 = [&](int l, int m) { return std::sqrt((double)(l - m) * K(m) * (double)(l + m + 1) / K(m + 1)); };
    auto nq2 = [&](int l, int m) {
        return std::sqrt((double)(l + m + 2) * (double)(l + m + 1) * (double)(2 * l + 1) * K(m) / ((double)(2 * l + 3) * K(m + 1)));
    };
    tab.clear();
    tab.reserve((size_t)(d + 1) * (d + 2) / 2 * 8);
    for (int M = 1; M <= d + 1; ++M)
        for (int L = M; L <= d + 1; ++L) {
            double e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (L == M) e[0] = diag[M];
            else if (L == M + 1) e[0] = sd[M + 1] / diag[M];
            else { e[0] = n1(L, M); e[1] = n2(L, M); }
            if (L <= d) {
                e[2] = M * cbar[idx(L, M)];
                e[3] = M * sbar[idx(L, M)];
                const double q = nq1(L, M - 1);
                e[4] = q * cbar[idx(L, M - 1)];
                e[5] = q * sbar[idx(L, M - 1)];
            }
            if (L >= 2) {
                const double q = nq2(L - 1, M - 1);
                e[6] = q * cbar[idx(L - 1, M - 1)];
                e[7] = q * sbar[idx(L - 1, M - 1)];
            }
            tab.insert(tab.end(), e, e + 8);
        }
    tab.insert(tab.end(), 16, 0.0);   // spare entries: the kernel's software pipeline reads ahead
}

// Stream of the DPP-broadcast form (bsk_device.hpp: gravity_sh_dpp): same iteration order, 8 doubles
// per entry, but (i) the recursion is rescaled column by column, Bt_L = B_L / alpha_L with
// alpha_M = alpha_(M+1) = 1, alpha_L = n2(L, M) alpha_(L-2), so entry[0] = n1 alpha_(L-1) / alpha_L is
// the only recursion constant and the six coefficient products carry alpha_L; (ii) every column is
// padded to an even number of entries (a 128-byte chunk = 2 entries never straddles a column);
// (iii) the stream is padded to whole SH_RING-chunk bodies plus two bodies of read-ahead slack.
// The walk is cut into two halves of (nearly) equal entry count at a column boundary: `split` is the first
// column of the second half, `chunk1` its first chunk; the kernels add the halves' partial sums in a fixed
// order whether one wave or two walk them.
ShLayout build_sh_table_dpp(int d, const double* cbar, const double* sbar, std::vector<double>& tab) {
    auto K = [](int i) { return i == 0 ? 1.0L : 2.0L; };
    auto idx = [](int l, int m) { return l * (l + 1) / 2 + m; };
    std::vector<long double> diag(d + 2), sd(d + 2), alpha(d + 3);
    diag[0] = 1.0L;
    for (int l = 1; l <= d + 1; ++l) diag[l] = sqrtl((long double)(2 * l + 1) * K(l) / ((long double)(2 * l) * K(l - 1))) * diag[l - 1];
    for (int l = 1; l <= d + 1; ++l) sd[l] = sqrtl((long double)(2 * l) * K(l - 1) / K(l)) * diag[l];
    auto n1 = [](int l, int m) { return sqrtl((long double)(2 * l + 1) * (long double)(2 * l - 1) / ((long double)(l - m) * (long double)(l + m))); };
    auto n2 = [](int l, int m) {
        return sqrtl((long double)(l + m - 1) * (long double)(2 * l + 1) * (long double)(l - m - 1) /
                     ((long double)(l + m) * (long double)(l - m) * (long double)(2 * l - 3)));
    };
    auto nq1 = [&](int l, int m) { return sqrtl((long double)(l - m) * K(m) * (long double)(l + m + 1) / K(m + 1)); };
    auto nq2 = [&](int l, int m) {
        return sqrtl((long double)(l + m + 2) * (long double)(l + m + 1) * (long double)(2 * l + 1) * K(m) /
                     ((long double)(2 * l + 3) * K(m + 1)));
    };
    tab.clear();
    std::vector<size_t> col_chunk(d + 3, 0);   // first chunk of column M
    for (int M = 1; M <= d + 1; ++M) {
        col_chunk[M] = tab.size() / 16;
        for (int L = M; L <= d + 1; ++L) {
            long double e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            alpha[L] = (L <= M + 1) ? 1.0L : n2(L, M) * alpha[L - 2];
            if (L == M) e[0] = diag[M];
            else if (L == M + 1) e[0] = sd[M + 1] / diag[M];
            else e[0] = n1(L, M) * alpha[L - 1] / alpha[L];
            if (L <= d) {
                e[2] = M * (long double)cbar[idx(L, M)];
                e[3] = M * (long double)sbar[idx(L, M)];
                const long double q = nq1(L, M - 1);
                e[4] = q * cbar[idx(L, M - 1)];
                e[5] = q * sbar[idx(L, M - 1)];
            }
            if (L >= 2) {
                const long double q = nq2(L - 1, M - 1);
                e[6] = q * cbar[idx(L - 1, M - 1)];
                e[7] = q * sbar[idx(L - 1, M - 1)];
            }
            for (int k = 0; k < 8; ++k) tab.push_back((double)(k >= 2 ? e[k] * alpha[L] : e[k]));
        }
        if ((d + 1 - M + 1) & 1) tab.insert(tab.end(), 8, 0.0);   // odd column: one all-zero entry
    }
    const size_t chunks = tab.size() / 16, R = bsk::SH_RING;
    col_chunk[d + 2] = chunks;
    ShLayout lay;
    // Balance the halves by issue slots, not by chunks: a column end costs about two chunks' worth (flush,
    // combine, restart, two taken branches) and the second half has many short columns; it also raises
    // (s + i t) to its first column's power first (about a third of a chunk per column skipped).
    auto cost0 = [&](int sp) { return (double)col_chunk[sp] + 2.0 * (sp - 1); };
    auto cost1 = [&](int sp) { return (double)(chunks - col_chunk[sp]) + 2.0 * (d + 2 - sp) + 0.33 * (sp - 1); };
    lay.split = 2;                                   // 1 < split <= d + 1: both halves own at least one column
    while (lay.split < d + 1 && cost0(lay.split + 1) <= cost1(lay.split + 1)) ++lay.split;
    lay.chunk1 = (int)col_chunk[lay.split];
    lay.bodies = (int)((chunks + R - 1) / R);
    lay.bodies0 = (int)((col_chunk[lay.split] + R - 1) / R);
    lay.bodies1 = (int)((chunks - col_chunk[lay.split] + R - 1) / R);
    tab.resize(((size_t)lay.bodies * R + 2 * R) * 16, 0.0);
    return lay;
}

int build_params(const bsk_config& c, bsk::StepParams& p, bsk::ColdCfg& k, bool& diag) {
    std::memset(&p, 0, sizeof p);
    std::memset(&k, 0, sizeof k);
    p.dt = c.dt;
    p.mu = c.mu;
    p.j2k = 1.5 * c.j2 * c.mu * c.req * c.req;
    std::memcpy(p.inertia, c.inertia, sizeof p.inertia);
    std::memcpy(k.inertia, c.inertia, sizeof k.inertia);
    double D[9];
    std::memcpy(D, c.inertia, sizeof D);
    for (int i = 0; i < c.n_rw; ++i) {
        double nrm = std::sqrt(c.gs[i][0] * c.gs[i][0] + c.gs[i][1] * c.gs[i][1] + c.gs[i][2] * c.gs[i][2]);
        if (!(std::fabs(nrm - 1.0) < 1e-9)) return fail(BSK_EINVAL, "wheel spin axis is not a unit vector");
        if (!(c.js[i] > 0.0)) return fail(BSK_EINVAL, "wheel inertia js must be positive");
        for (int a = 0; a < 3; ++a) {
            p.gs[i][a] = c.gs[i][a];
            for (int b = 0; b < 3; ++b) D[3 * a + b] -= c.js[i] * c.gs[i][a] * c.gs[i][b];
        }
        p.js[i] = c.js[i];
    }
    if (!inv3(D, p.dinv)) return fail(BSK_EINVAL, "hub inertia minus wheel inertia is singular");
    for (int i = 0; i < 9; ++i) { p.dmat[i] = D[i]; p.wmat[i] = c.inertia[i] - D[i]; }
    // Diagonal fast path: only when every off-diagonal of I_sc and of (I_sc - sum Js g g^T) is
    // EXACTLY zero (true for the reference's cuboid hub with the triad or the symmetric pyramid).
    diag = true;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            if (a != b && (c.inertia[3 * a + b] != 0.0 || D[3 * a + b] != 0.0)) diag = false;
    if (c.n_rw > 0) {
        // rwMotorTorque: map = CGs^T (CGs CGs^T)^-1 C,  CGs = C Gs
        double cgs[3][BSK_MAX_RW], M[9] = {0}, Mi[9];
        for (int a = 0; a < 3; ++a)
            for (int i = 0; i < c.n_rw; ++i)
                cgs[a][i] = c.ctrl_axes[3 * a] * c.gs[i][0] + c.ctrl_axes[3 * a + 1] * c.gs[i][1] +
                            c.ctrl_axes[3 * a + 2] * c.gs[i][2];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                for (int i = 0; i < c.n_rw; ++i) M[3 * a + b] += cgs[a][i] * cgs[b][i];
        if (!inv3(M, Mi)) return fail(BSK_EINVAL, "wheel set does not span the control axes");
        for (int i = 0; i < c.n_rw; ++i) {
            double t[3];
            for (int a = 0; a < 3; ++a) t[a] = cgs[0][i] * Mi[a] + cgs[1][i] * Mi[3 + a] + cgs[2][i] * Mi[6 + a];
            for (int b = 0; b < 3; ++b)
                k.map[i][b] = t[0] * c.ctrl_axes[b] + t[1] * c.ctrl_axes[3 + b] + t[2] * c.ctrl_axes[6 + b];
        }
    }
    p.f_coulomb = c.f_coulomb;
    p.fsw_every = c.fsw_every;
    p.fsw_lag = c.fsw_lag;
    p.nav_lag = c.nav_lag;
    p.req = c.req;
    p.planet_rate = c.planet_rate;
    p.sh_tab = nullptr;
    p.sh_degree = 0;
    p.sh_split = 2;
    p.sh_bodies = p.sh_bodies0 = p.sh_bodies1 = p.sh_chunk1 = 0;
    const bool full = (c.flags & (BSK_FLAG_SUN_THIRD_BODY | BSK_FLAG_DRAG | BSK_FLAG_DESAT)) != 0;
    p.ex.desat = (c.flags & BSK_FLAG_DESAT) ? 1 : 0;
    p.ex.pad_ = 0;
    k.n_thr = c.n_thr;
    k.hs_min = c.hs_min;
    k.inv_max_thrust = c.thr_max_thrust > 0.0 ? 1.0 / c.thr_max_thrust : 0.0;
    k.thr_min_fire_time = c.thr_min_fire_time;
    k.thr_min_on_time = c.thr_min_on_time;
    k.thr_max_counter = c.thr_max_counter;
    k.fsw_lag = c.fsw_lag;
    k.nav_lag = c.nav_lag;
    for (int i = 0; i < c.n_rw; ++i) { k.js[i] = c.js[i]; for (int j = 0; j < 3; ++j) k.gs[i][j] = c.gs[i][j]; }
    if (c.flags & BSK_FLAG_DESAT) {
        double dd[9] = {0}, ddi[9], Dm[BSK_MAX_THR][3];
        for (int i = 0; i < c.n_thr; ++i) {
            const double* r = c.thr_pos[i];
            const double* g = c.thr_dir[i];
            Dm[i][0] = r[1] * g[2] - r[2] * g[1]; Dm[i][1] = r[2] * g[0] - r[0] * g[2]; Dm[i][2] = r[0] * g[1] - r[1] * g[0];
            for (int j = 0; j < 3; ++j) { k.thr_f[i][j] = c.thr_max_thrust * g[j]; k.thr_l[i][j] = c.thr_max_thrust * Dm[i][j]; }
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) dd[3 * a + b] += Dm[i][a] * Dm[i][b];
        }
        if (!inv3(dd, ddi)) return fail(BSK_EINVAL, "thruster set does not span the three torque axes");
        for (int i = 0; i < c.n_thr; ++i)
            for (int a = 0; a < 3; ++a) k.thr_map[i][a] = ddi[3 * a] * Dm[i][0] + ddi[3 * a + 1] * Dm[i][1] + ddi[3 * a + 2] * Dm[i][2];
    }
    p.feat = full ? bsk::FEAT_FULL : ((c.flags & BSK_FLAG_POWER) ? bsk::FEAT_POWER : bsk::FEAT_BARE);   // FEAT_FULLG: below
    if (c.flags & BSK_FLAG_LDS_SCRATCH) p.feat = bsk::FEAT_LDSS;
    p.ex.mu_sun = (c.flags & BSK_FLAG_SUN_THIRD_BODY) ? c.mu_sun : 0.0;
    p.ex.base_density = (c.flags & BSK_FLAG_DRAG) ? c.base_density : 0.0;
    p.ex.inv_scale_height = c.scale_height > 0.0 ? 1.0 / c.scale_height : 0.0;
    p.ex.inv_mass = c.mass > 0.0 ? 1.0 / c.mass : 0.0;
    p.ex.rho_skip = 1e-25;
    k.n_facets = c.n_facets;
    k.facet_axis = 1;
    for (int i = 0; i < c.n_facets && i < 8; ++i) {
        // axis-aligned normal: exactly one component is +-1, the others exactly 0
        int axis = -1, nz = 0;
        for (int j = 0; j < 3; ++j)
            if (c.facet_normal[i][j] != 0.0) { ++nz; axis = j; }
        if (nz != 1 || std::fabs(c.facet_normal[i][axis]) != 1.0) { k.facet_axis = 0; break; }
        const int sgn = c.facet_normal[i][axis] > 0.0 ? 0 : 1;
        const double acd = c.facet_area[i] * c.facet_cd[i];
        k.fa_c[sgn][axis] += acd;
        for (int j = 0; j < 3; ++j) k.fa_r[sgn][axis][j] += acd * c.facet_pos[i][j];
    }
    // half sums / half differences of the +e_k and -e_k tables (bsk_device.hpp: facet_drag)
    for (int axis = 0; axis < 3; ++axis) {
        const double cp = k.fa_c[0][axis], cm = k.fa_c[1][axis];
        k.fa_c[0][axis] = 0.5 * (cp + cm);
        k.fa_c[1][axis] = 0.5 * (cp - cm);
        for (int j = 0; j < 3; ++j) {
            const double rp = k.fa_r[0][axis][j], rm = k.fa_r[1][axis][j];
            k.fa_r[0][axis][j] = 0.5 * (rp + rm);
            k.fa_r[1][axis][j] = 0.5 * (rp - rm);
        }
    }
    if (k.facet_axis) {
        bool diagonal = true;
        for (int sgn = 0; sgn < 2; ++sgn)
            for (int axis = 0; axis < 3; ++axis)
                for (int j = 0; j < 3; ++j)
                    if (j != axis && k.fa_r[sgn][axis][j] != 0.0) diagonal = false;
        if (diagonal) k.facet_axis = 2;   // facet centres on their own normal axes: 12 table values suffice
    }
    // any other facet set with live drag runs the generic-geometry variant of the full-scenario kernel
    if (full && (c.flags & BSK_FLAG_DRAG) && c.base_density != 0.0 && k.facet_axis != 2) p.feat = bsk::FEAT_FULLG;
    for (int i = 0; i < 8; ++i) {
        k.facet_acd[i] = c.facet_area[i] * c.facet_cd[i];
        for (int j = 0; j < 3; ++j) { k.facet_n[i][j] = c.facet_normal[i][j]; k.facet_r[i][j] = c.facet_pos[i][j]; }
    }
    {
        const double AU = 149597870700.0, RSUN = 695000.0e3;
        for (int i = 0; i < 3; ++i) { p.pc.nB[i] = c.panel_normal[i]; p.pc.sun_r0[i] = c.sun_r0[i]; p.pc.sun_v[i] = c.sun_v[i]; }
        p.pc.kflux = c.panel_area * c.panel_efficiency * c.solar_flux * AU * AU;
        p.pc.draw = c.power_draw;
        p.pc.cap = c.storage_capacity;
        p.pc.req = c.req;
        p.pc.rsun = RSUN;
        p.pc.rs_plus = RSUN + c.req;
        p.pc.rs_minus = RSUN - c.req;
    }
    k.u_max = c.u_max;
    k.u_min = c.u_min;
    k.K = c.K;
    k.P = c.P;
    std::memcpy(p.obs.sigma_R0N, c.sigma_R0N, sizeof p.obs.sigma_R0N);
    std::memcpy(k.sigma_R0N, c.sigma_R0N, sizeof k.sigma_R0N);
    p.obs.inv_wheel_limit = 1.0 / c.wheel_limit;
    p.obs.charge_scale = 1.0 / 3600.0 / c.power_max;
    p.obs.reward_mult = c.reward_mult;
    p.obs.failure_penalty = c.failure_penalty;
    p.obs.r_min2 = c.r_min * c.r_min;
    p.obs.max_length = c.max_length;
    p.obs.pad_ = 0;
    // broadcast table of the full-scenario kernels (bsk_device.hpp: KTab, KA_* / KB_* / KC_*)
    for (int i = 0; i < c.n_rw; ++i) {
        for (int j = 0; j < 3; ++j) k.kt[bsk::KA_G + 3 * i + j] = c.gs[i][j];
        k.kt[bsk::KA_JS + i] = c.js[i];
        k.kt[16 + bsk::KB_IJS + i] = 1.0 / c.js[i];
        for (int j = 0; j < 3; ++j) k.kt[48 + bsk::KD_JG + 3 * i + j] = c.js[i] * c.gs[i][j];
        k.kt[48 + bsk::KD_HIJS + i] = c.dt / c.js[i];
    }
    for (int sgn = 0; sgn < 2; ++sgn)
        for (int axis = 0; axis < 3; ++axis) {
            k.kt[16 + bsk::KB_FAC + 3 * sgn + axis] = k.fa_c[sgn][axis] * p.ex.inv_mass;   // area table carries 1/m
            k.kt[16 + bsk::KB_FAD + 3 * sgn + axis] = k.fa_r[sgn][axis][axis];
        }
    k.kt[32 + bsk::KC_IMASS] = p.ex.inv_mass;
    for (int j = 0; j < 3; ++j) k.kt[32 + bsk::KC_NB + j] = c.panel_normal[j];
    k.kt[32 + bsk::KC_KFLUX] = p.pc.kflux;
    k.kt[32 + bsk::KC_RHO0] = p.ex.base_density;
    k.kt[32 + bsk::KC_NIH] = -p.ex.inv_scale_height;
    k.kt[32 + bsk::KC_REQIH] = c.req * p.ex.inv_scale_height;
    k.kt[32 + bsk::KC_RSKIP] = p.ex.rho_skip;
    k.kt[32 + bsk::KC_LOG2E] = 1.4426950408889634074;
    k.kt[32 + bsk::KC_I6] = 1.0 / 6.0; k.kt[32 + bsk::KC_I24] = 1.0 / 24.0; k.kt[32 + bsk::KC_I120] = 1.0 / 120.0;   // Atmo::advance
    k.kt[32 + bsk::KC_I720] = 1.0 / 720.0;
    {   // row E: rho0 / k!, k = 0..13 (bsk_device.hpp: atmosphere_density), -ln2 split in two parts
        long double f = 1.0L;
        for (int i = 0; i < 14; ++i) {
            if (i > 1) f *= (long double)i;
            k.kt[64 + bsk::KE_POLY + i] = (double)((long double)p.ex.base_density / f);
        }
        k.kt[64 + bsk::KE_NLN2HI] = -6.93147180369123816490e-01;
        k.kt[64 + bsk::KE_NLN2LO] = -1.90821492927058770002e-10;
    }
    // thruster subset table: row m = sums over the set bits of m, ascending thruster index
    for (int m = 0; m < (1 << BSK_MAX_THR); ++m) {
        double f[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < c.n_thr && i < BSK_MAX_THR; ++i)
            if (m & (1 << i))
                for (int j = 0; j < 3; ++j) { f[j] += k.thr_f[i][j]; f[3 + j] += k.thr_l[i][j]; }
        for (int j = 0; j < 6; ++j) k.thr_tab[m][j] = f[j];
    }
    return BSK_OK;
}
int validate(const bsk_config& c) {
    if (c.abi_version != BSK_ABI_VERSION || c.struct_size != sizeof(bsk_config))
        return fail(BSK_EABI, "bsk_config abi_version/struct_size mismatch (header " + std::to_string(BSK_ABI_VERSION) +
                                  "/" + std::to_string(sizeof(bsk_config)) + ")");
    if (!(c.dt > 0.0)) return fail(BSK_EINVAL, "dt must be positive");
    if (c.fsw_every < 1 || c.fsw_every > 2047) return fail(BSK_EINVAL, "fsw_every must be in 1..2047");
    if (c.max_length < 0 || c.max_length > 1000000) return fail(BSK_EINVAL, "max_length must be in 0..1000000");
    if (c.fsw_lag != 0 && c.fsw_lag != 1) return fail(BSK_EINVAL, "fsw_lag must be 0 or 1");
    if (c.nav_lag != 0 && c.nav_lag != 1) return fail(BSK_EINVAL, "nav_lag must be 0 or 1");
    if (c.n_rw != 0 && c.n_rw != 3 && c.n_rw != 4) return fail(BSK_EINVAL, "n_rw must be 0, 3 or 4");
    if (c.gravity_model != BSK_GRAV_PM && c.gravity_model != BSK_GRAV_PM_J2 && c.gravity_model != BSK_GRAV_SH)
        return fail(BSK_EINVAL, "unknown gravity_model");
    if (c.gravity_model == BSK_GRAV_SH && (c.sh_degree < 2 || c.sh_degree > BSK_MAX_SH_DEGREE))
        return fail(BSK_EINVAL, "sh_degree must be in 2..70 for BSK_GRAV_SH");
    if ((c.flags & (BSK_FLAG_SUN_THIRD_BODY | BSK_FLAG_DRAG | BSK_FLAG_DESAT)) && !(c.flags & BSK_FLAG_POWER))
        return fail(BSK_EINVAL, "BSK_FLAG_SUN_THIRD_BODY / BSK_FLAG_DRAG / BSK_FLAG_DESAT are built in the full-scenario kernel: set BSK_FLAG_POWER too");
    if ((c.flags & BSK_FLAG_DESAT) && (c.n_thr < 3 || c.n_thr > BSK_MAX_THR || c.n_rw == 0 || !(c.thr_max_thrust > 0.0) || !(c.mass > 0.0)))
        return fail(BSK_EINVAL, "BSK_FLAG_DESAT needs 3..8 thrusters, wheels, thr_max_thrust > 0 and mass > 0");
    if ((c.flags & BSK_FLAG_DESAT) && !(std::isfinite(c.thr_min_on_time) && c.thr_min_on_time >= 0.0 && std::isfinite(c.thr_min_fire_time) && c.thr_min_fire_time >= 0.0))
        return fail(BSK_EINVAL, "BSK_FLAG_DESAT needs thr_min_on_time and thr_min_fire_time finite and not negative");
    // a burst limit is kept in 16 bits (bsk_device.hpp: desat_tick packs two per register): a stretched pulse must fit
    if ((c.flags & BSK_FLAG_DESAT) && !(std::floor(c.thr_min_on_time * (2.0 / c.dt)) <= 65535.0))
        return fail(BSK_EINVAL, "BSK_FLAG_DESAT: floor(thr_min_on_time * 2 / dt) must be at most 65535 (the burst limit of a pulse that passes "
                                "thr_min_fire_time and is stretched to thr_min_on_time, in half steps of dt, is kept in 16 bits)");
    if ((c.flags & BSK_FLAG_DRAG) && (c.n_facets < 0 || c.n_facets > 8 || !(c.scale_height > 0.0) || !(c.mass > 0.0)))
        return fail(BSK_EINVAL, "BSK_FLAG_DRAG needs 0..8 facets, scale_height > 0 and mass > 0");
    if ((c.flags & BSK_FLAG_LDS_SCRATCH) && ((c.flags & BSK_FLAG_POWER) || c.gravity_model == BSK_GRAV_SH))
        return fail(BSK_EINVAL, "BSK_FLAG_LDS_SCRATCH is built for the bare propagator (point mass / J2, no power system) only");
    if (!(c.mu > 0.0) || !(c.req > 0.0)) return fail(BSK_EINVAL, "mu and req must be positive");
    if (!(c.wheel_limit > 0.0) || !(c.power_max > 0.0)) return fail(BSK_EINVAL, "wheel_limit and power_max must be positive");
    if ((c.flags & BSK_FLAG_POWER) && !(c.storage_capacity > 0.0 && c.sun_r0[0] * c.sun_r0[0] + c.sun_r0[1] * c.sun_r0[1] + c.sun_r0[2] * c.sun_r0[2] > 0.0))
        return fail(BSK_EINVAL, "BSK_FLAG_POWER needs storage_capacity > 0 and a Sun position");
    return BSK_OK;
}
} }  // namespace bsk::capi

using namespace bsk::capi;

extern "C" {

int bsk_default_config(bsk_config* c, int n_rw, int gravity_model) {
    if (!c) return fail(BSK_EINVAL, "cfg is NULL");
    if (n_rw != 0 && n_rw != 3 && n_rw != 4) return fail(BSK_EINVAL, "n_rw must be 0, 3 or 4");
    std::memset(c, 0, sizeof *c);
    c->abi_version = BSK_ABI_VERSION;
    c->struct_size = sizeof *c;
    c->dt = 0.1;
    c->fsw_every = 10;
    c->gravity_model = gravity_model;
    c->sh_degree = 0;
    c->n_rw = n_rw;
    c->flags = 0;
    c->max_length = 540;
    c->fsw_lag = 1;
    c->nav_lag = 1;
    c->mu = 0.3986004415e15;
    c->req = 6378136.6;
    c->j2 = std::sqrt(5.0) * 4.841693e-4;
    c->planet_rate = 7.2921159e-5;
    const double m = 330.0, w = 1.38, dpt = 1.04, ht = 1.58;
    c->mass = m;
    c->inertia[0] = 1. / 12. * m * (w * w + dpt * dpt);
    c->inertia[4] = 1. / 12. * m * (dpt * dpt + ht * ht);
    c->inertia[8] = 1. / 12. * m * (w * w + ht * ht);
    const double D2R = M_PI / 180.0;
    if (n_rw == 3) {
        for (int i = 0; i < 3; ++i) c->gs[i][i] = 1.0;
    } else if (n_rw == 4) {
        // one quadrant's components with explicit signs: exactly symmetric set (see
        // actuatorPrimatives.balancedHR16Pyramid), so sum(g g^T) is exactly diagonal
        const double el = 40.0 * D2R, az = 45.0 * D2R;
        double cx = std::cos(az) * std::cos(el), cy = std::sin(az) * std::cos(el), cz = std::sin(el);
        const double nn = std::sqrt(cx * cx + cy * cy + cz * cz);
        cx /= nn; cy /= nn; cz /= nn;
        const int sx[4] = {1, -1, -1, 1}, sy[4] = {1, 1, -1, -1};
        for (int i = 0; i < 4; ++i) {
            c->gs[i][0] = sx[i] * cx;
            c->gs[i][1] = sy[i] * cy;
            c->gs[i][2] = cz;
        }
    }
    for (int i = 0; i < n_rw; ++i) c->js[i] = 50.0 / (6000.0 * M_PI * 2.0 / 60.0);
    c->u_max = 0.2;
    c->u_min = 0.00001;
    c->f_coulomb = 0.0005;
    c->K = 7.0;
    c->P = 35.0;
    c->sigma_R0N[0] = 1.0;
    c->ctrl_axes[0] = c->ctrl_axes[4] = c->ctrl_axes[8] = 1.0;
    c->wheel_limit = 3000.0 * (2.0 * M_PI / 60.0);
    c->power_max = 20.0;
    c->reward_mult = 1.0 / 540.0;
    c->failure_penalty = 1.0;
    c->r_min = 6378.1366 / 1000.0;
    c->panel_normal[1] = -1.0;
    c->panel_area = 0.2 * 0.3;
    c->panel_efficiency = 0.20;
    c->power_draw = -5.0;
    c->storage_capacity = 20.0 * 3600.0;
    c->solar_flux = 1372.5398;
    // epoch 2021 MAY 04 07:47:48.965 UTC (JD 2459338.5 + 07:47:48.965)
    const double jd0 = 2459338.5 + (7.0 * 3600.0 + 47.0 * 60.0 + 48.965) / 86400.0;
    double p0[3], p1[3];
    sun_position(jd0, p0);
    sun_position(jd0 + 1.0, p1);
    for (int k = 0; k < 3; ++k) {
        c->sun_r0[k] = p0[k];
        c->sun_v[k] = (p1[k] - p0[k]) / 86400.0;
    }
    c->mu_sun = 1.32712440018e20;
    c->hs_min = 4.0;
    c->thr_max_counter = 4;
    c->thr_min_fire_time = 0.002;
    {   // idealMonarc1Octet (actuatorPrimatives.py:66-161), MOOG Monarc-1: 0.9 N, MinOnTime 0.02 s
        const double x = 3.874945160902288e-2, y = 1.206182747348013, z = 0.85245, x2 = 3.8749451609022656e-2;
        const double loc[8][3] = {{x, -y, z}, {x, -y, -z}, {-x2, -y, z}, {-x2, -y, -z}, {-x, y, z}, {-x, y, -z}, {x2, y, z}, {x2, y, -z}};
        const double a = 0.7071067811865476, b = 0.7071067811865475;
        const double dir[8][3] = {{-a, b, 0}, {-a, b, 0}, {b, a, 0}, {b, a, 0}, {a, -b, 0}, {a, -b, 0}, {-b, -a, 0}, {-b, -a, 0}};
        c->n_thr = 8;
        for (int i = 0; i < 8; ++i)
            for (int k = 0; k < 3; ++k) { c->thr_pos[i][k] = loc[i][k]; c->thr_dir[i][k] = dir[i][k]; }
        c->thr_max_thrust = 0.9;
        c->thr_min_on_time = 0.020;
    }
    c->base_density = 1.22;
    c->scale_height = 8.0e3;
    // 6U cubesat facets + two 1x2 m panels, Cd 2.2 (leoPowerAttitudeSimulator.py:272-281)
    const double fa[8] = {0.2 * 0.3, 0.2 * 0.3, 0.1 * 0.2, 0.1 * 0.2, 0.1 * 0.3, 0.1 * 0.3, 1. * 2., 1. * 2.};
    const double fn[8][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {0, 1, 0}, {0, -1, 0}};
    const double fp[8][3] = {{0.05, 0, 0}, {0.05, 0, 0}, {0, 0.15, 0}, {0, -0.15, 0}, {0, 0, 0.1}, {0, 0, -0.1}, {0, 2., 0}, {0, 2., 0}};
    c->n_facets = 8;
    for (int i = 0; i < 8; ++i) {
        c->facet_area[i] = fa[i];
        c->facet_cd[i] = 2.2;
        for (int k = 0; k < 3; ++k) { c->facet_normal[i][k] = fn[i][k]; c->facet_pos[i][k] = fp[i][k]; }
    }
    return BSK_OK;
}
}  // extern "C"
