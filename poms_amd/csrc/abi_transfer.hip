// extern "C" boundary of libpoms_hip.so (declared in include/poms_hip.h): the transfer
// object -- restriction, prolongation, the fused residual -> restriction -- and the
// dense coarse-grid mat-vec.
#include "common.hpp"
#include "launchers.hpp"
#include "split_hooks.hpp"
#include "abi_internal.hpp"
#include "../../include/poms_hip.h"

#include <algorithm>
#include <vector>

using namespace poms;

extern "C" {

// ---- transfer -------------------------------------------------------------------
int poms_transfer_create(poms_ctx* ctx, int ndim, const poms_layout* fine, int64_t g0,
                         const int64_t* nf_global, const int64_t* nc, const double* const* P,
                         poms_transfer** tr) {
    if (!ctx || !tr || !nf_global || !nc || !P || !layout_ok(fine)) {
        set_error("poms_transfer_create: bad argument");
        return 1;
    }
    if (ndim < 1 || ndim > 3) { set_error("poms_transfer_create: ndim 1..3"); return 1; }
    const bool is3d = ndim == 3;
    const int d0 = is3d ? 0 : 1;
    int64_t ncmax = 0;
    for (int d = d0; d < 3; ++d) {
        if (!P[d] || nc[d] < 1 || nf_global[d] < 1) { set_error("poms_transfer_create: bad axis"); return 1; }
        ncmax = std::max(ncmax, nc[d]);
    }
    if (!is3d && (fine->n[0] != 1 || fine->pads[0] != 0)) {
        set_error("poms_transfer_create: 1D/2D layouts need n[0]=1, pads[0]=0");
        return 1;
    }
    for (int d = 1; d < 3; ++d)
        if (nf_global[d] != fine->n[d]) { set_error("poms_transfer_create: only axis 0 may be sliced"); return 1; }
    if (is3d && (g0 < 0 || g0 + fine->n[0] > nf_global[0])) { set_error("poms_transfer_create: bad slab"); return 1; }
    POMS_HIP_CHECK(hipSetDevice(ctx->device));
    auto* t = new poms_transfer();
    t->ctx = ctx;
    t->ndim = ndim;
    t->ncm = ncmax <= 16 ? 16 : 32;
    t->banded = ncmax > 32;
    t->L = *fine;
    t->g0 = is3d ? g0 : 0;
    int rc = 0;
    for (int d = 0; d < 3; ++d) {
        t->nf[d] = (d < d0) ? 1 : nf_global[d];
        t->nc[d] = (d < d0) ? 1 : nc[d];
        if (d < d0) continue;
        if (!t->banded) {
            std::vector<double> pm(t->nf[d] * t->ncm, 0.0);
            for (int64_t i = 0; i < t->nf[d]; ++i)
                for (int64_t j = 0; j < t->nc[d]; ++j) pm[i * t->ncm + j] = P[d][i * t->nc[d] + j];
            rc |= upload(pm.data(), pm.size(), &t->Pm[d]);
            continue;
        }
        // banded: non-zero span of every row of P and of every column
        const int64_t nfd = t->nf[d], ncd = t->nc[d];
        const double* Pd = P[d];
        std::vector<int> jl(nfd, 0), il(ncd, 0);
        int wp = 1, wr = 1;
        for (int64_t i = 0; i < nfd; ++i) {
            int64_t a = -1, b = -1;
            for (int64_t j = 0; j < ncd; ++j)
                if (Pd[i * ncd + j] != 0.0) { if (a < 0) a = j; b = j; }
            jl[i] = a < 0 ? 0 : (int)a;
            wp = std::max(wp, a < 0 ? 1 : (int)(b - a + 1));
        }
        for (int64_t j = 0; j < ncd; ++j) {
            int64_t a = -1, b = -1;
            for (int64_t i = 0; i < nfd; ++i)
                if (Pd[i * ncd + j] != 0.0) { if (a < 0) a = i; b = i; }
            il[j] = a < 0 ? 0 : (int)a;
            wr = std::max(wr, a < 0 ? 1 : (int)(b - a + 1));
        }
        if (wp > 64 || wr > 256) { set_error("poms_transfer_create: prolongation is not banded"); rc = 1; break; }
        std::vector<double> pb(nfd * wp, 0.0), rb(ncd * wr, 0.0);
        for (int64_t i = 0; i < nfd; ++i)
            for (int k = 0; k < wp && jl[i] + k < ncd; ++k) pb[i * wp + k] = Pd[i * ncd + jl[i] + k];
        for (int64_t j = 0; j < ncd; ++j)
            for (int k = 0; k < wr && il[j] + k < nfd; ++k) rb[j * wr + k] = Pd[(il[j] + k) * ncd + j];
        t->wP[d] = wp;
        t->wR[d] = wr;
        rc |= upload(pb.data(), pb.size(), &t->Pb[d]);
        rc |= upload(rb.data(), rb.size(), &t->Rb[d]);
        if (!rc && hipMalloc(reinterpret_cast<void**>(&t->jlo[d]), nfd * sizeof(int)) != hipSuccess) rc = 1;
        if (!rc && hipMalloc(reinterpret_cast<void**>(&t->ilo[d]), ncd * sizeof(int)) != hipSuccess) rc = 1;
        if (!rc && hipMemcpy(t->jlo[d], jl.data(), nfd * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) rc = 1;
        if (!rc && hipMemcpy(t->ilo[d], il.data(), ncd * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) rc = 1;
    }
    const int64_t n1 = fine->n[1], n2 = fine->n[2];
    const size_t sz0 = (size_t)t->nc[0] * n1 * n2;
    const size_t sz1 = (size_t)t->nc[0] * t->nc[1] * n2;
    if (!rc && hipMalloc(reinterpret_cast<void**>(&t->t0), std::max<size_t>(sz0, 1) * sizeof(double)) != hipSuccess) rc = 1;
    if (!rc && hipMalloc(reinterpret_cast<void**>(&t->t1), std::max<size_t>(sz1, 1) * sizeof(double)) != hipSuccess) rc = 1;
    if (rc) {
        if (!error_is_set()) set_error("poms_transfer_create: allocation failed");
        poms_transfer_destroy(t);
        return 1;
    }
    *tr = t;
    return 0;
}

int poms_transfer_destroy(poms_transfer* t) {
    if (!t) return 0;
    for (double* p : {t->Pm[0], t->Pm[1], t->Pm[2], t->t0, t->t1, t->Pb[0], t->Pb[1], t->Pb[2], t->Rb[0],
                      t->Rb[1], t->Rb[2], t->part, t->Gf[0], t->Gf[1], t->Gf[2], t->Gf[3], t->Gf[4], t->Gf[5],
                      t->Pf[0], t->Pf[1], t->Pf[2], t->ru, t->rv, t->mpart})
        if (p) (void)hipFree(p);
    for (int* p : {t->jlo[0], t->jlo[1], t->jlo[2], t->ilo[0], t->ilo[1], t->ilo[2]})
        if (p) (void)hipFree(p);
    delete t;
    return 0;
}

// one axis pass of a transfer: dense-P kernels for small coarse extents, banded
// gather kernels otherwise
static int tpass(poms_transfer* t, bool restrict_dir, int d, const AxisPass& ps, const double* in,
                 double* out, hipStream_t st) {
    if (!t->banded) {
        double* part = nullptr;
        if (restrict_dir) {   // split-axis partials (few lines): a buffer grown on first use
            const int64_t need = transfer_split_scratch(t->ncm, ps);
            if (need > t->part_n) {
                if (t->part) (void)hipFree(t->part);
                t->part = nullptr;
                t->part_n = 0;
                if (hipMalloc(reinterpret_cast<void**>(&t->part), need * sizeof(double)) != hipSuccess) {
                    set_error("transfer: partial-sum buffer allocation failed");
                    return 1;
                }
                t->part_n = need;
            }
            part = t->part;
        }
        return transfer_pass_launch(restrict_dir, t->ncm, ps, t->Pm[d], in, out, st, part);
    }
    return restrict_dir ? transfer_band_launch(true, ps, t->Rb[d], t->ilo[d], t->wR[d], in, out, st)
                        : transfer_band_launch(false, ps, t->Pb[d], t->jlo[d], t->wP[d], in, out, st);
}

int poms_restrict(poms_transfer* t, const double* fine, double* coarse, void* stream) {
    if (!t || !fine || !coarse) { set_error("poms_restrict: null argument"); return 1; }
    const RowGeom g = row_geom(&t->L);
    const int64_t n0 = g.n0, n1 = g.n1, n2 = g.n2;
    const int64_t c0 = t->nc[0], c1 = t->nc[1], c2 = t->nc[2];
    hipStream_t st = as_stream(stream);
    const int64_t fbase = (int64_t)g.pd0 * g.s0 + (int64_t)g.pd1 * g.s1 + g.pd2;
    const double* src1;  // input of the axis-1 pass (dense [c0][n1][n2] or the fine vector)
    AxisPass a1{};
    if (t->ndim == 3) {
        AxisPass a0{};
        a0.nA = 1; a0.nB1 = n1; a0.nB2 = n2;
        a0.in_base = fbase; a0.in_sb1 = g.s1; a0.in_sb2 = 1; a0.in_si = g.s0;
        a0.out_sb1 = n2; a0.out_sb2 = 1; a0.out_si = n1 * n2;
        a0.nI = (int)n0; a0.nJ = (int)c0; a0.goff = (int)t->g0;
        if (tpass(t, true, 0, a0, fine, t->t0, st)) return 1;
        src1 = t->t0;
        a1.nA = c0; a1.nB1 = 1; a1.nB2 = n2;
        a1.in_base = 0; a1.in_sa = n1 * n2; a1.in_sb2 = 1; a1.in_si = n2;
    } else {
        src1 = fine;
        a1.nA = 1; a1.nB1 = 1; a1.nB2 = n2;
        a1.in_base = fbase; a1.in_sb2 = 1; a1.in_si = g.s1;
    }
    a1.out_sa = c1 * n2; a1.out_sb2 = 1; a1.out_si = n2;
    a1.nI = (int)n1; a1.nJ = (int)c1; a1.goff = 0;
    if (tpass(t, true, 1, a1, src1, t->t1, st)) return 1;
    AxisPass a2{};
    a2.nA = c0 * c1; a2.nB1 = 1; a2.nB2 = 1;
    a2.in_sa = n2; a2.in_si = 1;
    a2.out_sa = c2; a2.out_si = 1;
    a2.nI = (int)n2; a2.nJ = (int)c2; a2.goff = 0;
    if (tpass(t, true, 2, a2, t->t1, coarse, st)) return 1;
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_prolong_add(poms_transfer* t, const double* coarse, double* fine, void* stream) {
    if (!t || !fine || !coarse) { set_error("poms_prolong_add: null argument"); return 1; }
    const RowGeom g = row_geom(&t->L);
    const int64_t n0 = g.n0, n1 = g.n1, n2 = g.n2;
    const int64_t c0 = t->nc[0], c1 = t->nc[1], c2 = t->nc[2];
    hipStream_t st = as_stream(stream);
    const int64_t fbase = (int64_t)g.pd0 * g.s0 + (int64_t)g.pd1 * g.s1 + g.pd2;
    // axis 2: coarse [c0*c1][c2] -> t1 [c0*c1][n2]
    AxisPass a2{};
    a2.nA = c0 * c1; a2.nB1 = 1; a2.nB2 = 1;
    a2.in_sa = c2; a2.in_si = 1; a2.nJ = (int)c2;
    a2.out_sa = n2; a2.out_si = 1; a2.nI = (int)n2; a2.goff = 0; a2.accumulate = 0;
    if (tpass(t, false, 2, a2, coarse, t->t1, st)) return 1;
    // axis 1: t1 [c0][c1][n2] -> t0 [c0][n1][n2] (3D) or fine (2D, accumulate)
    AxisPass a1{};
    a1.nA = c0; a1.nB1 = 1; a1.nB2 = n2;
    a1.in_sa = c1 * n2; a1.in_sb2 = 1; a1.in_si = n2; a1.nJ = (int)c1;
    a1.nI = (int)n1; a1.goff = 0;
    if (t->ndim == 3) {
        a1.out_sa = n1 * n2; a1.out_sb2 = 1; a1.out_si = n2; a1.accumulate = 0;
        if (tpass(t, false, 1, a1, t->t1, t->t0, st)) return 1;
        AxisPass a0{};
        a0.nA = 1; a0.nB1 = n1; a0.nB2 = n2;
        a0.in_sb1 = n2; a0.in_sb2 = 1; a0.in_si = n1 * n2; a0.nJ = (int)c0;
        a0.out_base = fbase; a0.out_sb1 = g.s1; a0.out_sb2 = 1; a0.out_si = g.s0;
        a0.nI = (int)n0; a0.goff = (int)t->g0; a0.accumulate = 1;
        if (tpass(t, false, 0, a0, t->t0, fine, st)) return 1;
    } else {
        a1.out_base = fbase; a1.out_sb2 = 1; a1.out_si = g.s1; a1.accumulate = 1;
        if (tpass(t, false, 1, a1, t->t1, fine, st)) return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- fused residual -> restriction ------------------------------------------------
static void plan_resid_restrict(poms_transfer* t, bool sum);

// G[r] are HOST dense row-major (rows of axis d x nc_d) matrices F_r^T P_d, one per
// operator role in poms_op_create's factor order (A0 M0 A1 B1 M2 K2 for FORM_SUM,
// F0 - F1 - F2 - for FORM_SINGLE; 2D: roles 0, 1 unused).  Rows as P's: axis 0 global
// (3D), axes 1 and 2 the transfer's own.
int poms_transfer_set_operator(poms_transfer* t, int form, const double* const* G) {
    if (!t || !G || (form != FORM_SUM && form != FORM_SINGLE)) {
        set_error("poms_transfer_set_operator: bad argument");
        return 1;
    }
    if (t->banded) { set_error("poms_transfer_set_operator: coarse extents > 32 (banded transfer)"); return 1; }
    const bool is3d = t->ndim == 3;
    const bool sum = form == FORM_SUM;
    int64_t ncmax = 1;
    for (int d = 0; d < 3; ++d) ncmax = std::max(ncmax, t->nc[d]);
    const int ncf = ncmax <= 8 ? 8 : ncmax <= 12 ? 12 : ncmax <= 16 ? 16 : 32;
    for (int r = 0; r < 6; ++r) {
        const bool need = (r / 2 > 0 || is3d) && (sum || r % 2 == 0);
        if (need && !G[r]) { set_error("poms_transfer_set_operator: missing factor"); return 1; }
    }
    POMS_HIP_CHECK(hipSetDevice(t->ctx->device));
    for (double*& p : t->Gf) { if (p) (void)hipFree(p); p = nullptr; }
    for (double*& p : t->Pf) { if (p) (void)hipFree(p); p = nullptr; }
    if (t->ru) (void)hipFree(t->ru);
    if (t->rv) (void)hipFree(t->rv);
    if (t->mpart) (void)hipFree(t->mpart);
    t->ru = t->rv = t->mpart = nullptr;
    t->mpart_n = 0;
    t->nrpass = 0;
    t->rform = -1;
    int rc = 0;
    auto pad = [&](const double* src, int d, double sign, double** dev) {
        std::vector<double> m(t->nf[d] * ncf, 0.0);
        for (int64_t i = 0; i < t->nf[d]; ++i)
            for (int64_t j = 0; j < t->nc[d]; ++j) m[i * ncf + j] = sign * src[i * t->nc[d] + j];
        return upload(m.data(), m.size(), dev);
    };
    for (int r = 0; r < 6 && !rc; ++r) {
        const int d = r / 2;
        if ((d == 0 && !is3d) || !G[r] || (!sum && r % 2)) continue;
        rc |= pad(G[r], d, d == 2 ? -1.0 : 1.0, &t->Gf[r]);
    }
    // P padded to ncf: the transfer keeps only its own (16 / 32-column) copy on the device
    for (int d = is3d ? 0 : 1; d < 3 && !rc; ++d) {
        std::vector<double> pm(t->nf[d] * t->ncm);
        if (hipMemcpy(pm.data(), t->Pm[d], pm.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = 1;
            break;
        }
        std::vector<double> pc(t->nf[d] * t->nc[d]);
        for (int64_t i = 0; i < t->nf[d]; ++i)
            for (int64_t j = 0; j < t->nc[d]; ++j) pc[i * t->nc[d] + j] = pm[i * t->ncm + j];
        rc |= pad(pc.data(), d, 1.0, &t->Pf[d]);
    }
    const int64_t n1 = t->L.n[1], n2 = t->L.n[2];
    const size_t su = (size_t)t->nc[0] * n1 * n2, sv = (size_t)t->nc[0] * t->nc[1] * n2;
    if (!rc && hipMalloc(reinterpret_cast<void**>(&t->ru), 3 * std::max<size_t>(su, 1) * sizeof(double)) != hipSuccess) rc = 1;
    if (!rc && hipMalloc(reinterpret_cast<void**>(&t->rv), 3 * std::max<size_t>(sv, 1) * sizeof(double)) != hipSuccess) rc = 1;
    // the call's passes, and their chunk partials once at the largest pass's need
    int64_t need = 0;
    if (!rc) {
        plan_resid_restrict(t, sum);
        for (int i = 0; i < t->nrpass; ++i) need = std::max(need, mrestrict_scratch(t->rpass[i], ncf));
    }
    if (!rc && need > 0 && hipMalloc(reinterpret_cast<void**>(&t->mpart), need * sizeof(double)) != hipSuccess) rc = 1;
    if (rc) {
        if (!error_is_set()) set_error("poms_transfer_set_operator: allocation failed");
        return 1;
    }
    t->mpart_n = need;
    t->ncf = ncf;
    t->rform = form;
    return 0;
}

// coarse = R (b - A x), local slab contribution (the caller all-reduces).  Three
// passes (2D: two); the FORM_SUM factorisation shares its axis-0 and axis-1 outputs:
//   u_a = G_A0 x, u_m = G_M0 x, u_c = P0 b                          (axis 0)
//   v_1 = G_A1 u_a + G_B1 u_m, v_2 = G_A1 u_m, v_3 = P1 u_c           (axis 1)
//   coarse = P2 v_3 - G_M2 v_1 - G_K2 v_2                            (axis 2)
// since A = A0 (x) A1 (x) M2 + M0 (x) B1 (x) M2 + M0 (x) A1 (x) K2 (2D: A1 (x) M2 +
// B1 (x) K2; FORM_SINGLE: F0 (x) F1 (x) F2).  x needs no ghost planes: each fine
// row enters through its own row of G.
// Everything of the passes that is fixed once the operator is set goes into t->rpass
// here (from Gf, Pf, ru, rv): x and b, the first pass's in[0] and in[1], and coarse, the
// last pass's out[0], stay null for poms_resid_restrict to fill in.
static void plan_resid_restrict(poms_transfer* t, bool sum) {
    const RowGeom g = row_geom(&t->L);
    const int64_t n0 = g.n0, n1 = g.n1, n2 = g.n2;
    const int64_t c0 = t->nc[0], c1 = t->nc[1], c2 = t->nc[2];
    const int64_t fbase = (int64_t)g.pd0 * g.s0 + (int64_t)g.pd1 * g.s1 + g.pd2;
    const size_t su = (size_t)c0 * n1 * n2, sv = (size_t)c0 * c1 * n2;
    double* u[3] = {t->ru, t->ru + su, t->ru + 2 * su};
    double* v[3] = {t->rv, t->rv + sv, t->rv + 2 * sv};
    double* const* G = t->Gf;
    t->nrpass = 0;
    // the axis-2 pass (the last) reads w[0..2] with w[0] = the P-chain of b
    auto last = [&](const double* wb, const double* w1, const double* w2, const AxisPass& a2) {
        MultiPass& mp = t->rpass[t->nrpass++] = MultiPass{};
        mp.ps = a2;
        mp.ni = sum ? 3 : 2;
        mp.no = 1;
        mp.in[0] = wb; mp.in[1] = w1; mp.in[2] = sum ? w2 : nullptr;
        mp.m[0][0] = t->Pf[2];
        mp.m[0][1] = G[4];
        mp.m[0][2] = sum ? G[5] : nullptr;
    };
    AxisPass a2{};
    a2.nA = c0 * c1; a2.nB1 = 1; a2.nB2 = 1;
    a2.in_sa = n2; a2.in_si = 1;
    a2.out_sa = c2; a2.out_si = 1;
    a2.nI = (int)n2; a2.nJ = (int)c2; a2.goff = 0;
    if (t->ndim == 3) {
        MultiPass& mp = t->rpass[t->nrpass++] = MultiPass{};
        AxisPass& a0 = mp.ps;
        a0.nA = 1; a0.nB1 = n1; a0.nB2 = n2;
        a0.in_base = fbase; a0.in_sb1 = g.s1; a0.in_sb2 = 1; a0.in_si = g.s0;
        a0.out_sb1 = n2; a0.out_sb2 = 1; a0.out_si = n1 * n2;
        a0.nI = (int)n0; a0.nJ = (int)c0; a0.goff = (int)t->g0;
        mp.ni = 2;   // x, b
        // outputs: u_c (b), u_a, [u_m]
        mp.no = sum ? 3 : 2;
        mp.out[0] = u[0]; mp.out[1] = u[1]; mp.out[2] = u[2];
        mp.m[0][1] = t->Pf[0];
        mp.m[1][0] = G[0];
        if (sum) mp.m[2][0] = G[1];
        MultiPass& m1 = t->rpass[t->nrpass++] = MultiPass{};
        AxisPass& a1 = m1.ps;
        a1.nA = c0; a1.nB1 = 1; a1.nB2 = n2;
        a1.in_base = 0; a1.in_sa = n1 * n2; a1.in_sb2 = 1; a1.in_si = n2;
        a1.out_sa = c1 * n2; a1.out_sb2 = 1; a1.out_si = n2;
        a1.nI = (int)n1; a1.nJ = (int)c1; a1.goff = 0;
        m1.ni = sum ? 3 : 2;
        m1.in[0] = u[0]; m1.in[1] = u[1]; m1.in[2] = u[2];
        m1.no = sum ? 3 : 2;
        m1.out[0] = v[0]; m1.out[1] = v[1]; m1.out[2] = v[2];
        m1.m[0][0] = t->Pf[1];              // v_3 (here v[0]) = P1 u_c
        m1.m[1][1] = G[2];                  // v_1 = G_A1 u_a + G_B1 u_m
        if (sum) {
            m1.m[1][2] = G[3];
            m1.m[2][2] = G[2];              // v_2 = G_A1 u_m
        }
        last(v[0], v[1], v[2], a2);
    } else {
        MultiPass& mp = t->rpass[t->nrpass++] = MultiPass{};
        AxisPass& a1 = mp.ps;
        a1.nA = 1; a1.nB1 = 1; a1.nB2 = n2;
        a1.in_base = fbase; a1.in_sb2 = 1; a1.in_si = g.s1;
        a1.out_sa = c1 * n2; a1.out_sb2 = 1; a1.out_si = n2;
        a1.nI = (int)n1; a1.nJ = (int)c1; a1.goff = 0;
        mp.ni = 2;   // x, b
        mp.no = sum ? 3 : 2;
        mp.out[0] = v[0]; mp.out[1] = v[1]; mp.out[2] = v[2];
        mp.m[0][1] = t->Pf[1];              // P1 b
        mp.m[1][0] = G[2];                  // G_A1 x (-> M2)
        if (sum) mp.m[2][0] = G[3];         // G_B1 x (-> K2)
        last(v[0], v[1], v[2], a2);
    }
}

// The planned passes with this call's x, b and coarse; no allocation (the call may be
// captured into a graph).
int poms_resid_restrict(poms_transfer* t, const double* b, const double* x, double* coarse, void* stream) {
    if (!t || !b || !x || !coarse) { set_error("poms_resid_restrict: null argument"); return 1; }
    if (t->rform < 0) { set_error("poms_resid_restrict: no operator set (poms_transfer_set_operator)"); return 1; }
    for (int i = 0; i < t->nrpass; ++i) {
        MultiPass mp = t->rpass[i];
        if (i == 0) { mp.in[0] = x; mp.in[1] = b; }
        if (i == t->nrpass - 1) mp.out[0] = coarse;
        if (mrestrict_scratch(mp, t->ncf) > t->mpart_n) {
            set_error("poms_resid_restrict: a pass needs more partials than poms_transfer_set_operator planned");
            return 1;
        }
        if (mrestrict_launch(t->ncf, mp, t->mpart, as_stream(stream))) return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_dense_matvec(poms_ctx* ctx, int64_t n, const double* Minv, const double* x, double* y,
                      void* stream) {
    if (!ctx || !Minv || !x || !y || n < 1 || n > (1 << 20)) { set_error("dense_matvec: bad argument"); return 1; }
    dense_matvec_launch((int)n, Minv, x, y, as_stream(stream));
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
