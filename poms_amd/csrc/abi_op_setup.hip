// Operators are made and unmade here, once each (declared in include/poms_hip.h): the
// Kronecker forms' factor upload and Toeplitz ranges, the stored stencil, the assembled
// stencil, the matrix-free form with its table checks and launch geometry, the Galerkin
// product, the host copies, destroy.  abi_op.hip has everything that runs per launch.
#include "common.hpp"
#include "launchers.hpp"
#include "split_hooks.hpp"
#include "abi_internal.hpp"
#include "../../include/poms_hip.h"

#include <algorithm>
#include <vector>

using namespace poms;

// Largest row range [lo, hi) around the middle whose band rows equal one
// symmetric row (bitwise), for the pair (fa, fb) (fb may be null).
static void toeplitz_range(const double* fa, const double* fb, int64_t n, int P, int* lo, int* hi,
                           double* ta, double* tb) {
    const int W = 2 * P + 1;
    *lo = *hi = 0;
    for (int j = 0; j < 6; ++j) { ta[j] = 0.0; tb[j] = 0.0; }
    if (n < 1) return;
    const int64_t m = n / 2;
    auto sym = [&](const double* f) {
        if (!f) return true;
        for (int j = 1; j <= P; ++j)
            if (f[m * W + P + j] != f[m * W + P - j]) return false;
        return true;
    };
    if (!sym(fa) || !sym(fb)) return;
    auto same = [&](int64_t i) {
        for (int k = 0; k < W; ++k) {
            if (fa[i * W + k] != fa[m * W + k]) return false;
            if (fb && fb[i * W + k] != fb[m * W + k]) return false;
        }
        return true;
    };
    int64_t a = m, b = m + 1;
    while (a > 0 && same(a - 1)) --a;
    while (b < n && same(b)) ++b;
    *lo = (int)a;
    *hi = (int)b;
    for (int j = 0; j <= P; ++j) {
        ta[j] = fa[m * W + P + j];
        tb[j] = fb ? fb[m * W + P + j] : 0.0;
    }
}

// A new general-form operator (FORM_STENCIL, FORM_MATFREE) on `layout`: its half-widths
// are the layout's pads; the slab start g0 and the global axis-0 extent count in 3D only.
static poms_op* new_general_op(poms_ctx* ctx, int ndim, int form, const poms_layout* layout, int64_t g0,
                               int64_t n0_global) {
    auto* o = new poms_op();
    o->ctx = ctx;
    o->ndim = ndim;
    o->form = form;
    o->L = *layout;
    o->g0 = ndim == 3 ? g0 : 0;
    o->n0g = ndim == 3 ? n0_global : 1;
    for (int d = 0; d < 3; ++d) o->sp[d] = (int)layout->pads[d];
    o->pmax = std::max(o->sp[0], std::max(o->sp[1], o->sp[2]));
    return o;
}

// The axes a 1D / 2D operator does not use have n = 1 and no pads; else the error is set.
static bool leading_axes_ok(const std::string& prefix, int ndim, const poms_layout* layout) {
    for (int d = 0; d < 3 - ndim; ++d)
        if (layout->n[d] != 1 || layout->pads[d] != 0) {
            set_error(prefix + "unused leading axes need n = 1, pads = 0");
            return false;
        }
    return true;
}

// A device temporary of `bytes` (at least 8), remembered on `owned` for the caller to free,
// also after a failure (null); h not null: filled from the host.
static void* dev_tmp(std::vector<void*>& owned, const void* h, size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(bytes, 8)) != hipSuccess) return nullptr;
    owned.push_back(d);
    if (h && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

// A set-up launch on the null stream was accepted and has run.
static bool setup_launch_done() { return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess; }

// The per-axis quadrature tables on the device as ax[3]; an unused leading axis gets one
// element with one point of weight 1 and the constant function.  Every allocation goes
// onto `owned`, which the caller frees, also after a failure (returns 1).
static int upload_axes(int ndim, const int* nel, const int* nq, const int* p, const int* const* first,
                       const int* const* es, const int* const* ee, const double* const* basis,
                       const double* const* weights, const int64_t* nglob, AssembleAxis* ax,
                       std::vector<void*>& owned) {
    auto up = [&](const void* h, size_t bytes) { return dev_tmp(owned, h, bytes); };
    static const int zero_i = 0;
    static const double unit_b[2] = {1.0, 0.0}, unit_w = 1.0;
    for (int d = 0; d < 3; ++d) {
        const bool used = d >= 3 - ndim;
        const int ne = used ? nel[d] : 1, q = used ? nq[d] : 1, pp = used ? p[d] : 0;
        const int64_t n = used ? nglob[d] : 1;
        AssembleAxis& A = ax[d];
        A.first = static_cast<const int*>(up(used ? first[d] : &zero_i, ne * sizeof(int)));
        A.es = static_cast<const int*>(up(used ? es[d] : &zero_i, n * sizeof(int)));
        A.ee = static_cast<const int*>(up(used ? ee[d] : &zero_i, n * sizeof(int)));
        A.basis = static_cast<const double*>(up(used ? basis[d] : unit_b, (size_t)ne * q * (pp + 1) * 2 * sizeof(double)));
        A.w = static_cast<const double*>(up(used ? weights[d] : &unit_w, (size_t)ne * q * sizeof(double)));
        A.nel = ne; A.nq = q; A.p = pp; A.n = (int)n;
        if (!A.first || !A.es || !A.ee || !A.basis || !A.w) return 1;
    }
    return 0;
}

// On-device assembly of -div(a grad u) + c u into a FORM_STENCIL operator; tensor: a_q
// holds the ndim (ndim + 1) / 2 component planes of a tensor coefficient.
static int assemble_stencil_impl(const std::string& fn, poms_ctx* ctx, int ndim, const poms_layout* layout,
                                 const int* nel, const int* nq, const int* p, const int* const* first,
                                 const int* const* es, const int* const* ee, const double* const* basis,
                                 const double* const* weights, const int64_t* nglob, const double* a_q, bool tensor,
                                 const double* c_q, double mass_coef, int64_t g0, poms_op** op) {
    if (!ctx || !op || !layout_ok(layout) || !nel || !nq || !p || !first || !es || !ee || !basis || !weights || !nglob) {
        set_error(fn + ": bad argument");
        return 1;
    }
    if (ndim < 1 || ndim > 3) { set_error(fn + ": ndim 1..3"); return 1; }
    if (!leading_axes_ok(fn + ": ", ndim, layout)) return 1;
    for (int d = 3 - ndim; d < 3; ++d) {
        if (p[d] != layout->pads[d] || nel[d] < 1 || nq[d] < 1 || !first[d] || !es[d] || !ee[d] || !basis[d] ||
            !weights[d]) {
            set_error(fn + ": axis " + std::to_string(d) + " (degree must equal the pad)");
            return 1;
        }
        if (d > 0 && nglob[d] != layout->n[d]) { set_error(fn + ": only axis 0 may be sliced"); return 1; }
    }
    if (ndim == 3 && (g0 < 0 || g0 + layout->n[0] > nglob[0])) { set_error(fn + ": bad slab"); return 1; }
    POMS_HIP_CHECK(hipSetDevice(ctx->device));
    const RowGeom r = row_geom(layout);
    const int64_t W = (int64_t)(2 * r.pd0 + 1) * (2 * r.pd1 + 1) * (2 * r.pd2 + 1);
    const int64_t cst = (int64_t)r.n0 * r.n1 * r.n2;
    poms_op* o = new_general_op(ctx, ndim, FORM_STENCIL, layout, g0, nglob[0]);
    std::vector<void*> tmp;
    AssembleAxis ax[3];
    int rc = upload_axes(ndim, nel, nq, p, first, es, ee, basis, weights, nglob, ax, tmp);
    if (!rc && hipMalloc(reinterpret_cast<void**>(&o->coef), std::max<int64_t>(W * cst, 1) * sizeof(double)) != hipSuccess)
        rc = 1;
    if (!rc) {
        assemble_launch(ax, (int)o->g0, r.n0, a_q, c_q, mass_coef, o->coef, nullptr, tensor ? ndim : 0);
        if (!setup_launch_done()) rc = 1;
    }
    for (void* d : tmp) (void)hipFree(d);
    if (rc) {
        set_error(fn + ": allocation, upload or launch failed");
        poms_op_destroy(o);
        return 1;
    }
    *op = o;
    return 0;
}

// The matrix-free form of -div(a grad u) + c u (csrc/matfree.hip).  The kernel indexes
// with the tables unguarded: every check comes first, before any device call.  tensor:
// a_q holds the ncomp component planes of a tensor coefficient (not null).
static int create_matfree_impl(const std::string& name, poms_ctx* ctx, int ndim, const poms_layout* layout,
                               const int* nel, const int* nq, const int* p, const int* const* first,
                               const int* const* es, const int* const* ee, const double* const* basis,
                               const double* const* weights, const int64_t* nglob, const double* a_q, bool tensor,
                               int ncomp, const double* c_q, double mass_coef, poms_op** op) {
    const std::string fn = name + ": ";
    if (!ctx || !op || !layout || !nel || !nq || !p || !first || !es || !ee || !basis || !weights || !nglob ||
        (tensor && !a_q)) {
        set_error(fn + "null argument");
        return 1;
    }
    if (ndim != 2 && ndim != 3) { set_error(fn + "ndim must be 2 or 3"); return 1; }
    if (tensor && ncomp != ndim * (ndim + 1) / 2) {
        set_error(fn + "ncomp must be d (d + 1) / 2 = " + std::to_string(ndim * (ndim + 1) / 2) + ", got " +
                  std::to_string(ncomp));
        return 1;
    }
    if (!layout_ok(layout)) { set_error(fn + "bad layout"); return 1; }
    if (layout->flags & POMS_LAYOUT_GHOST_DATA) {
        set_error(fn + "distributed operators (slabs, Cart blocks) are not supported");
        return 1;
    }
    if (!leading_axes_ok(fn, ndim, layout)) return 1;
    const int T = matfree_tile();
    for (int d = 3 - ndim; d < 3; ++d) {
        const std::string ax = "axis " + std::to_string(d) + ": ";
        if (!first[d] || !es[d] || !ee[d] || !basis[d] || !weights[d]) { set_error(fn + ax + "null table"); return 1; }
        if (p[d] < 1 || p[d] > 3) { set_error(fn + ax + "degree must be 1..3"); return 1; }
        if (p[d] != layout->pads[d]) { set_error(fn + ax + "degree must equal the layout's pad"); return 1; }
        if (nq[d] < 1 || nq[d] > 5) { set_error(fn + ax + "quadrature points per element must be 1..5"); return 1; }
        if (nglob[d] != layout->n[d]) {
            set_error(fn + ax + "distributed operators are not supported (nglob must equal the layout's extent)");
            return 1;
        }
        const int64_t n = nglob[d];
        if (n > 0x3fffffffLL || nel[d] < 1 || nel[d] > n) { set_error(fn + ax + "bad element count or extent"); return 1; }
        const int ne = nel[d], pp = p[d];
        for (int e = 0; e < ne; ++e)
            if (first[d][e] < 0 || first[d][e] + pp >= n || (e > 0 && first[d][e] < first[d][e - 1])) {
                set_error(fn + ax + "first[" + std::to_string(e) + "] outside its range or decreasing");
                return 1;
            }
        for (int64_t i = 0; i < n; ++i) {
            const int a = es[d][i], b = ee[d][i];
            bool ok = a >= 0 && b < ne && a <= b && (i == 0 || (a >= es[d][i - 1] && b >= ee[d][i - 1]));
            // every element of the support holds the function among its p+1
            for (int e = a; ok && e <= b; ++e) ok = i >= first[d][e] && i <= first[d][e] + pp;
            if (!ok) { set_error(fn + ax + "es / ee of basis function " + std::to_string(i) + " outside their range"); return 1; }
        }
        // every tile's window and element range fit the kernel's LDS arrays
        for (int64_t lo = 0; lo < n; lo += T) {
            const int64_t hi = std::min<int64_t>(lo + T, n);
            const int ea = es[d][lo], eb = ee[d][hi - 1];
            if (eb - ea + 1 > matfree_max_elements() || first[d][eb] + pp + 1 - first[d][ea] > matfree_max_window()) {
                set_error(fn + ax + "a tile's element range or window exceeds the kernel's limits");
                return 1;
            }
        }
    }
    const int64_t ndof = layout->n[0] * layout->n[1] * layout->n[2];
    if (ndof > ((int64_t)1 << 36)) { set_error(fn + "grid too large"); return 1; }
    POMS_HIP_CHECK(hipSetDevice(ctx->device));
    if (tensor) {
        std::string why;
        if (!matfree_tensor_builds_ok(&why)) { set_error(fn + why); return 1; }
    }
    const RowGeom r = row_geom(layout);
    poms_op* o = new_general_op(ctx, ndim, FORM_MATFREE, layout, 0, nglob[0]);
    o->mf_a = a_q;
    o->mf_tensor = tensor;
    o->mf_c = c_q;
    o->mf_mass = mass_coef;
    int rc = upload_axes(ndim, nel, nq, p, first, es, ee, basis, weights, nglob, o->mf_ax, o->mf_tabs);
    if (!rc && hipMalloc(reinterpret_cast<void**>(&o->mf_diag), std::max<int64_t>(ndof, 1) * sizeof(double)) != hipSuccess)
        rc = 1;
    if (!rc) {
        matfree_diag_launch(o->mf_ax, a_q, c_q, mass_coef, o->mf_diag, nullptr, tensor ? ndim : 0);
        if (!setup_launch_done()) rc = 1;
    }
    if (rc) {
        set_error(fn + "allocation, upload or launch failed");
        poms_op_destroy(o);
        return 1;
    }
    // launch geometry: 3D marches chunks of axis 0, at least 16 planes each; the number
    // of chunks with the fewest plane steps over whole rounds of the 512 workgroups the
    // 256 CUs hold (two per CU at 63 KB of LDS each), a chunk costing its planes + p0
    MatfreeGeom& g = o->mf_geom;
    g.s0 = r.s0; g.s1 = r.s1;
    g.n0 = r.n0; g.n1 = r.n1; g.n2 = r.n2;
    g.pd0 = r.pd0; g.pd1 = r.pd1; g.pd2 = r.pd2;
    g.tiles1 = (r.n1 + T - 1) / T;
    g.tiles2 = (r.n2 + T - 1) / T;
    const int64_t t12 = (int64_t)g.tiles1 * g.tiles2;
    int64_t want = 1;
    double best = 1e300;
    for (int64_t nc = 1; nc <= std::max(1, r.n0 / 16); ++nc) {
        const double cost = (double)((t12 * nc + 511) / 512) * (double)((r.n0 + nc - 1) / nc + r.pd0);
        if (cost < best - 1e-9) { best = cost; want = nc; }
    }
    g.chunk = (int)((r.n0 + want - 1) / want);
    g.nchunks = (r.n0 + g.chunk - 1) / g.chunk;
    g.ntiles = t12 * g.nchunks;
    *op = o;
    return 0;
}

extern "C" {

int poms_op_create(poms_ctx* ctx, int ndim, const poms_layout* layout, int form, int pmax,
                   const double* const* f, int64_t g0, int64_t n0_global, poms_op** op) {
    if (!ctx || !op || !f) { set_error("poms_op_create: null argument"); return 1; }
    if (ndim < 1 || ndim > 3) { set_error("poms_op_create: ndim must be 1..3"); return 1; }
    if (pmax < 1 || pmax > 5) { set_error("poms_op_create: pmax must be 1..5"); return 1; }
    if (form != FORM_SUM && form != FORM_SINGLE) { set_error("poms_op_create: bad form"); return 1; }
    if (!layout_ok(layout)) { set_error("poms_op_create: bad layout"); return 1; }
    const bool is3d = ndim == 3;
    if (!is3d && (layout->n[0] != 1 || layout->pads[0] != 0)) {
        set_error("poms_op_create: 1D/2D layouts need n[0]=1, pads[0]=0");
        return 1;
    }
    for (int d = 0; d < 3; ++d)
        if (layout->pads[d] > pmax) { set_error("poms_op_create: storage pad exceeds pmax"); return 1; }
    if (is3d && (g0 < 0 || g0 + layout->n[0] > n0_global)) {
        set_error("poms_op_create: slab [g0, g0+n0) outside [0, n0_global)");
        return 1;
    }
    const bool sum = form == FORM_SUM;
    if (!f[2] || !f[4] || (sum && (!f[3] || !f[5])) || (is3d && (!f[0] || (sum && !f[1])))) {
        set_error("poms_op_create: missing factor array");
        return 1;
    }
    POMS_HIP_CHECK(hipSetDevice(ctx->device));
    const int W = 2 * pmax + 1;
    auto* o = new poms_op();
    o->ctx = ctx;
    o->ndim = ndim;
    o->form = form;
    o->pmax = pmax;
    o->L = *layout;
    o->g0 = is3d ? g0 : 0;
    o->n0g = is3d ? n0_global : 1;
    o->ghost_corners = (layout->flags & POMS_LAYOUT_GHOST_DATA) != 0;
    int rc = 0;
    if (is3d) {
        // Transposed (column) bands of the axis-0 factors, padded by pmax rows on
        // both sides: at[(j+P)*W + s] = F[j-P+s][2P-s].
        const int64_t nrow = n0_global + 2 * pmax;
        std::vector<double> ta(nrow * W, 0.0), tb(nrow * W, 0.0);
        for (int64_t j = -pmax; j < n0_global + pmax; ++j)
            for (int s = 0; s < W; ++s) {
                const int64_t i = j - pmax + s;
                if (i < 0 || i >= n0_global) continue;
                ta[(j + pmax) * W + s] = f[0][i * W + (2 * pmax - s)];
                if (sum) tb[(j + pmax) * W + s] = f[1][i * W + (2 * pmax - s)];
            }
        rc |= upload(ta.data(), ta.size(), &o->a0t);
        if (sum) rc |= upload(tb.data(), tb.size(), &o->b0t);
    }
    rc |= upload(f[2], (size_t)layout->n[1] * W, &o->a1);
    rc |= upload(f[4], (size_t)layout->n[2] * W, &o->a2);
    if (sum) {
        rc |= upload(f[3], (size_t)layout->n[1] * W, &o->b1);
        rc |= upload(f[5], (size_t)layout->n[2] * W, &o->b2);
    }
    {
        std::vector<double> da(layout->n[2]), db(layout->n[2], 0.0);
        for (int64_t c = 0; c < layout->n[2]; ++c) {
            da[c] = f[4][c * W + pmax];
            if (sum) db[c] = f[5][c * W + pmax];
        }
        rc |= upload(da.data(), da.size(), &o->dg2a);
        rc |= upload(db.data(), db.size(), &o->dg2b);
    }
    if (rc) { poms_op_destroy(o); return 1; }
    // v2 preconditions: storage pads == pmax on the used axes
    o->v2_ok = layout->pads[1] == pmax && layout->pads[2] == pmax && (!is3d || layout->pads[0] == pmax);
    if (is3d)
        toeplitz_range(f[0], sum ? f[1] : nullptr, n0_global, pmax, &o->tc.lo0, &o->tc.hi0, o->tc.t0a, o->tc.t0b);
    toeplitz_range(f[2], sum ? f[3] : nullptr, layout->n[1], pmax, &o->tc.lo1, &o->tc.hi1, o->tc.t1a, o->tc.t1b);
    toeplitz_range(f[4], sum ? f[5] : nullptr, layout->n[2], pmax, &o->tc.lo2, &o->tc.hi2, o->tc.t2a, o->tc.t2b);
    o->variant = o->v2_ok ? 8 : 0;
    // 1/diag(A) on each global plane for points in the Toeplitz interior of axes 1
    // and 2 (same expression as the kernels' per-point diagonal)
    if (o->tc.lo1 < o->tc.hi1 && o->tc.lo2 < o->tc.hi2) {
        const double d1a = o->tc.t1a[0], d1b = sum ? o->tc.t1b[0] : 0.0;
        const double d2a = o->tc.t2a[0], d2b = sum ? o->tc.t2b[0] : 0.0;
        const int64_t np = is3d ? n0_global : 1;
        std::vector<double> rd(np);
        for (int64_t i = 0; i < np; ++i) {
            double dg;
            if (is3d) {
                const double d0a = f[0][i * W + pmax], d0b = sum ? f[1][i * W + pmax] : 0.0;
                dg = sum ? d0a * (d1a * d2a) + d0b * (d1b * d2a + d1a * d2b) : d0a * (d1a * d2a);
            } else {
                dg = sum ? d1a * d2a + d1b * d2b : d1a * d2a;
            }
            rd[i] = dg != 0.0 ? 1.0 / dg : 0.0;
        }
        if (upload(rd.data(), rd.size(), &o->rdiag0)) { poms_op_destroy(o); return 1; }
        // the same value on every plane of the axis-0 Toeplitz interior (bitwise: those
        // rows equal the middle row)
        if (is3d && o->tc.lo0 < o->tc.hi0) o->tc.rdi = rd[(o->tc.lo0 + o->tc.hi0) / 2];
    }
    *op = o;
    return 0;
}

int poms_op_create_stencil(poms_ctx* ctx, int ndim, const poms_layout* layout, const double* data,
                           int64_t g0, int64_t n0_global, poms_op** op) {
    if (!ctx || !op || !data || !layout_ok(layout)) { set_error("poms_op_create_stencil: bad argument"); return 1; }
    if (ndim < 1 || ndim > 3) { set_error("poms_op_create_stencil: ndim 1..3"); return 1; }
    if (!leading_axes_ok("poms_op_create_stencil: ", ndim, layout)) return 1;
    const RowGeom r = row_geom(layout);
    const int p[3] = {r.pd0, r.pd1, r.pd2};
    const int w[3] = {2 * p[0] + 1, 2 * p[1] + 1, 2 * p[2] + 1};
    const int64_t W = (int64_t)w[0] * w[1] * w[2];
    const int64_t cst = (int64_t)r.n0 * r.n1 * r.n2;
    if (W * cst * 8 > ((int64_t)1 << 40)) { set_error("poms_op_create_stencil: coefficients too large"); return 1; }
    POMS_HIP_CHECK(hipSetDevice(ctx->device));
    // spl layout: rows over the padded local extents, then the W offsets of each row
    const int64_t P1 = r.n1 + 2 * p[1], P2 = r.n2 + 2 * p[2];
    std::vector<double> soa((size_t)(W * cst));
    for (int64_t i0 = 0; i0 < r.n0; ++i0)
        for (int64_t i1 = 0; i1 < r.n1; ++i1)
            for (int64_t i2 = 0; i2 < r.n2; ++i2) {
                const int64_t row = ((i0 + p[0]) * P1 + (i1 + p[1])) * P2 + (i2 + p[2]);
                const int64_t lin = (i0 * r.n1 + i1) * r.n2 + i2;
                const double* src = data + row * W;
                for (int64_t k = 0; k < W; ++k) soa[(size_t)(k * cst + lin)] = src[k];
            }
    poms_op* o = new_general_op(ctx, ndim, FORM_STENCIL, layout, g0, n0_global);
    if (upload(soa.data(), soa.size(), &o->coef)) { poms_op_destroy(o); return 1; }
    *op = o;
    return 0;
}

int poms_op_assemble_stencil(poms_ctx* ctx, int ndim, const poms_layout* layout, const int* nel, const int* nq,
                             const int* p, const int* const* first, const int* const* es, const int* const* ee,
                             const double* const* basis, const double* const* weights, const int64_t* nglob,
                             const double* a_q, const double* c_q, double mass_coef, int64_t g0, poms_op** op) {
    return assemble_stencil_impl("poms_op_assemble_stencil", ctx, ndim, layout, nel, nq, p, first, es, ee, basis,
                                 weights, nglob, a_q, false, c_q, mass_coef, g0, op);
}

int poms_op_assemble_stencil_tensor(poms_ctx* ctx, int ndim, const poms_layout* layout, const int* nel, const int* nq,
                                    const int* p, const int* const* first, const int* const* es,
                                    const int* const* ee, const double* const* basis, const double* const* weights,
                                    const int64_t* nglob, const double* g_q, int ncomp, const double* c_q,
                                    double mass_coef, int64_t g0, poms_op** op) {
    const std::string fn = "poms_op_assemble_stencil_tensor";
    if (!ctx || !op || !layout || !nel || !nq || !p || !first || !es || !ee || !basis || !weights || !nglob || !g_q) {
        set_error(fn + ": null argument");
        return 1;
    }
    if (ndim < 1 || ndim > 3) { set_error(fn + ": ndim 1..3"); return 1; }
    if (ncomp != ndim * (ndim + 1) / 2) {
        set_error(fn + ": ncomp must be d (d + 1) / 2 = " + std::to_string(ndim * (ndim + 1) / 2) + ", got " +
                  std::to_string(ncomp));
        return 1;
    }
    return assemble_stencil_impl(fn, ctx, ndim, layout, nel, nq, p, first, es, ee, basis, weights, nglob, g_q, true,
                                 c_q, mass_coef, g0, op);
}

int poms_op_create_matfree(poms_ctx* ctx, int ndim, const poms_layout* layout, const int* nel, const int* nq,
                           const int* p, const int* const* first, const int* const* es, const int* const* ee,
                           const double* const* basis, const double* const* weights, const int64_t* nglob,
                           const double* a_q, const double* c_q, double mass_coef, poms_op** op) {
    return create_matfree_impl("poms_op_create_matfree", ctx, ndim, layout, nel, nq, p, first, es, ee, basis, weights,
                               nglob, a_q, false, 0, c_q, mass_coef, op);
}

int poms_op_create_matfree_tensor(poms_ctx* ctx, int ndim, const poms_layout* layout, const int* nel, const int* nq,
                                  const int* p, const int* const* first, const int* const* es, const int* const* ee,
                                  const double* const* basis, const double* const* weights, const int64_t* nglob,
                                  const double* g_q, int ncomp, const double* c_q, double mass_coef, poms_op** op) {
    return create_matfree_impl("poms_op_create_matfree_tensor", ctx, ndim, layout, nel, nq, p, first, es, ee, basis,
                               weights, nglob, g_q, true, ncomp, c_q, mass_coef, op);
}

int poms_op_diagonal(poms_op* o, double* diag_host) {
    if (!o || !diag_host) { set_error("poms_op_diagonal: null argument"); return 1; }
    const RowGeom r = row_geom(&o->L);
    const int64_t cst = (int64_t)r.n0 * r.n1 * r.n2;
    const double* src = nullptr;
    if (o->form == FORM_MATFREE) {
        src = o->mf_diag;
    } else if (o->form == FORM_STENCIL && o->coef) {   // the centre offset's coefficient plane
        const int w1 = 2 * o->sp[1] + 1, w2 = 2 * o->sp[2] + 1;
        src = o->coef + ((int64_t)(o->sp[0] * w1 + o->sp[1]) * w2 + o->sp[2]) * cst;
    } else {
        set_error("poms_op_diagonal: needs a matrix-free or general-stencil operator");
        return 1;
    }
    POMS_HIP_CHECK(hipMemcpy(diag_host, src, cst * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int poms_op_stencil_data(poms_op* o, double* data_host) {
    if (!o || !data_host || o->form != FORM_STENCIL) { set_error("poms_op_stencil_data: needs a general-stencil operator"); return 1; }
    const RowGeom r = row_geom(&o->L);
    const StencilGeom g = stencil_geom(r, o->sp, 0, 0, 0, 0, 0);   // (no planes, no mask: the whole operator as stored)
    const int64_t W = (int64_t)g.w0 * g.w1 * g.w2;
    const int64_t rows = (int64_t)(r.n0 + 2 * o->sp[0]) * (r.n1 + 2 * o->sp[1]) * (r.n2 + 2 * o->sp[2]);
    double* d = nullptr;
    POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), rows * W * sizeof(double)));
    int rc = 0;
    if (hipMemset(d, 0, rows * W * sizeof(double)) != hipSuccess) rc = 1;
    if (!rc) stencil_to_spl_launch(g, o->coef, d, nullptr);
    if (!rc && (hipGetLastError() != hipSuccess ||
                hipMemcpy(data_host, d, rows * W * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
        rc = 1;
    (void)hipFree(d);
    if (rc) { set_error("poms_op_stencil_data: copy failed"); return 1; }
    return 0;
}

// Galerkin coarse operator P^T A P of a general stencil (csrc/stencil_galerkin.hip).
// The passes index with the tables built here unguarded: every check comes first.
int poms_op_galerkin_stencil(poms_op* fine, const poms_layout* coarse_layout, const int64_t* nf, const int64_t* nc,
                             const double* const* P, poms_op** coarse) {
    const std::string fn = "poms_op_galerkin_stencil: ";
    if (!fine || !coarse_layout || !nf || !nc || !P || !coarse) { set_error(fn + "null argument"); return 1; }
    if (fine->form != FORM_STENCIL || !fine->coef) { set_error(fn + "needs a general-stencil operator"); return 1; }
    if (!layout_ok(coarse_layout)) { set_error(fn + "bad coarse layout"); return 1; }
    if (distributed(fine) || (coarse_layout->flags & POMS_LAYOUT_GHOST_DATA)) {
        set_error(fn + "distributed operators (slabs, Cart blocks) are not supported");
        return 1;
    }
    const int d0 = 3 - fine->ndim;
    int64_t wtot = 1;
    for (int d = 0; d < 3; ++d) {
        const std::string ax = "axis " + std::to_string(d) + ": ";
        if (!P[d]) { set_error(fn + ax + "null prolongation factor"); return 1; }
        if (nf[d] != fine->L.n[d]) { set_error(fn + ax + "nf does not match the fine operator's rows"); return 1; }
        if (nc[d] < 1 || nc[d] != coarse_layout->n[d]) { set_error(fn + ax + "nc does not match the coarse layout"); return 1; }
        if (coarse_layout->pads[d] != fine->sp[d]) {
            set_error(fn + ax + "the coarse pads must equal the fine stencil half-widths");
            return 1;
        }
        if (d < d0 && (nf[d] != 1 || nc[d] != 1)) { set_error(fn + ax + "unused leading axes need nf = nc = 1"); return 1; }
        if (fine->sp[d] < 0 || fine->sp[d] > 5) { set_error(fn + ax + "stencil half-width above 5"); return 1; }
        wtot *= 2 * fine->sp[d] + 1;
    }
    if (wtot * nf[0] * nf[1] * nf[2] * 8 > ((int64_t)1 << 40) || nf[0] * nf[1] * nf[2] > 0x7fffffffLL) {
        set_error(fn + "coefficients too large");
        return 1;
    }
    // per used axis: the row support [lo, lo + cnt) of every column, then the products
    // wt[I][ii][k][kc] = P[lo[I] + ii, I] P[lo[I] + ii + k - p, I + kc - p]
    std::vector<int> lo[3], cnt[3];
    std::vector<double> wt[3];
    int smax[3] = {1, 1, 1};
    for (int d = d0; d < 3; ++d) {
        const std::string ax = "axis " + std::to_string(d) + ": ";
        const int64_t m = nf[d], n = nc[d];
        const int p = fine->sp[d], w = 2 * p + 1;
        const double* Pd = P[d];
        lo[d].assign(n, 0);
        cnt[d].assign(n, 0);
        for (int64_t I = 0; I < n; ++I) {
            int64_t a = m, b = -1;
            for (int64_t i = 0; i < m; ++i)
                if (Pd[i * n + I] != 0.0) { a = std::min(a, i); b = i; }
            if (b < 0) { set_error(fn + ax + "column " + std::to_string(I) + " of P is empty"); return 1; }
            lo[d][I] = (int)a;
            cnt[d][I] = (int)(b - a + 1);
            smax[d] = std::max(smax[d], cnt[d][I]);
        }
        // columns more than p apart must not meet through a fine coupling (|i - j| <= p)
        for (int64_t I = 0; I < n; ++I)
            for (int64_t J = I + p + 1; J < n; ++J) {
                const int hiI = lo[d][I] + cnt[d][I] - 1, hiJ = lo[d][J] + cnt[d][J] - 1;
                if (std::max(lo[d][J] - hiI, lo[d][I] - hiJ) <= p) {
                    set_error(fn + ax + "coarse stencil would be wider than the layout's pads");
                    return 1;
                }
            }
        if ((int64_t)n * smax[d] * w * w > ((int64_t)1 << 27)) { set_error(fn + ax + "weight table too large"); return 1; }
        wt[d].assign((size_t)(n * smax[d] * w * w), 0.0);
        for (int64_t I = 0; I < n; ++I)
            for (int ii = 0; ii < cnt[d][I]; ++ii) {
                const int64_t i = lo[d][I] + ii;
                for (int k = 0; k < w; ++k) {
                    const int64_t j = i + k - p;
                    if (j < 0 || j >= m) continue;
                    for (int kc = 0; kc < w; ++kc) {
                        const int64_t J = I + kc - p;
                        if (J < 0 || J >= n) continue;
                        const int64_t e = ((int64_t)ii * w + k) * w + kc;
                        // (columns contiguous for the axis-2 pass, see GalerkinPass)
                        wt[d][(size_t)(d < 2 ? I * smax[d] * w * w + e : e * n + I)] = Pd[i * n + I] * Pd[j * n + J];
                    }
                }
            }
    }
    POMS_HIP_CHECK(hipSetDevice(fine->ctx->device));
    // (the coarse pads are the fine half-widths, checked above)
    poms_op* o = new_general_op(fine->ctx, fine->ndim, FORM_STENCIL, coarse_layout, 0, nc[0]);
    std::vector<void*> tmp;
    auto dev = [&](const void* h, size_t bytes) { return dev_tmp(tmp, h, bytes); };   // (h null: uninitialised)
    GalerkinPass ps[3];
    double* bufs[3] = {nullptr, nullptr, nullptr};   // output of each pass
    int np = 0, rc = 0;
    int64_t ext[3] = {nf[0], nf[1], nf[2]};
    for (int d = d0; d < 3 && !rc; ++d, ++np) {
        GalerkinPass& g = ps[np];
        g.d = d;
        for (int e = 0; e < 3; ++e) { g.w[e] = 2 * fine->sp[e] + 1; g.nin[e] = (int)ext[e]; }
        g.cst_in = ext[0] * ext[1] * ext[2];
        ext[d] = nc[d];
        for (int e = 0; e < 3; ++e) g.nout[e] = (int)ext[e];
        g.cst_out = ext[0] * ext[1] * ext[2];
        g.smax = smax[d];
        g.ws_col = d < 2 ? (int64_t)smax[d] * g.w[d] * g.w[d] : 1;
        g.ws_ent = d < 2 ? 1 : nc[d];
        g.lo = static_cast<const int*>(dev(lo[d].data(), lo[d].size() * sizeof(int)));
        g.cnt = static_cast<const int*>(dev(cnt[d].data(), cnt[d].size() * sizeof(int)));
        g.wt = static_cast<const double*>(dev(wt[d].data(), wt[d].size() * sizeof(double)));
        if (!g.lo || !g.cnt || !g.wt) rc = 1;
        if (!rc && d < 2) {   // an intermediate; the last pass writes the operator's planes
            bufs[np] = static_cast<double*>(dev(nullptr, (size_t)(wtot * g.cst_out) * sizeof(double)));
            if (!bufs[np]) rc = 1;
        }
    }
    if (!rc && hipMalloc(reinterpret_cast<void**>(&o->coef), (size_t)(wtot * nc[0] * nc[1] * nc[2]) * sizeof(double)) != hipSuccess)
        rc = 1;
    if (!rc) {
        const double* in = fine->coef;
        for (int s = 0; s < np && !rc; ++s) {
            double* out = s == np - 1 ? o->coef : bufs[s];
            rc = galerkin_pass_launch(ps[s], in, out, nullptr);
            in = out;
        }
        if (!setup_launch_done()) rc = 1;
    }
    for (void* p : tmp) (void)hipFree(p);
    if (rc) {
        set_error(fn + "allocation, upload or launch failed");
        poms_op_destroy(o);
        return 1;
    }
    *coarse = o;
    return 0;
}

int poms_op_destroy(poms_op* o) {
    if (!o) return 0;
    for (double* p : {o->a0t, o->b0t, o->a1, o->b1, o->a2, o->b2, o->dg2a, o->dg2b, o->rdiag0, o->coef, o->sv_dev,
                      o->spec_dev, o->spec_bak, o->la_raw, o->rf_raw})
        if (p) (void)hipFree(p);
    for (void* p : o->mf_tabs)
        if (p) (void)hipFree(p);
    if (o->mf_diag) (void)hipFree(o->mf_diag);
    for (const double* p : o->mf_faces.s)
        if (p) (void)hipFree(const_cast<double*>(p));
    for (double* p : {o->spec_part, o->spec_host})
        if (p) (void)hipHostFree(p);
    pcg_slots_free(o->sv);
    for (auto& g : o->spec_graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (o->cap_stream) (void)hipStreamDestroy(o->cap_stream);
    for (auto& t : o->tl) {
        (void)hipEventDestroy(t.e0);
        (void)hipEventDestroy(t.e1);
    }
    delete o;
    return 0;
}

int poms_kron_dot_2d(poms_ctx* ctx, const int64_t* starts, const int64_t* ends,
                     const int64_t* pads, const double* X, double* X_tmp, double* Y,
                     const double* A, int64_t a_rows, const double* B, int64_t b_rows) {
    (void)X_tmp;
    if (!ctx || !starts || !ends || !pads || !X || !Y || !A || !B) {
        set_error("poms_kron_dot_2d: null argument");
        return 1;
    }
    const int64_t n1 = ends[0] - starts[0] + 1, n2 = ends[1] - starts[1] + 1;
    const int p1 = (int)pads[0], p2 = (int)pads[1];
    if (n1 < 1 || n2 < 1 || p1 < 1 || p2 < 1 || p1 > 5 || p2 > 5) {
        set_error("poms_kron_dot_2d: bad extents or pads (1..5)");
        return 1;
    }
    if (starts[0] < 0 || ends[0] >= a_rows || starts[1] < 0 || ends[1] >= b_rows) {
        set_error("poms_kron_dot_2d: starts/ends outside the band arrays");
        return 1;
    }
    const int pm = std::max(p1, p2), W = 2 * pm + 1;
    // local, re-centred band rows of width 2*pm+1
    std::vector<double> fa(n1 * W, 0.0), fb(n2 * W, 0.0);
    for (int64_t i = 0; i < n1; ++i)
        for (int k = 0; k < 2 * p1 + 1; ++k) fa[i * W + k + pm - p1] = A[(starts[0] + i) * (2 * p1 + 1) + k];
    for (int64_t i = 0; i < n2; ++i)
        for (int k = 0; k < 2 * p2 + 1; ++k) fb[i * W + k + pm - p2] = B[(starts[1] + i) * (2 * p2 + 1) + k];
    poms_layout L{{1, n1, n2}, {0, p1, p2}};
    const double* f[6] = {nullptr, nullptr, fa.data(), nullptr, fb.data(), nullptr};
    poms_op* op = nullptr;
    if (poms_op_create(ctx, 2, &L, FORM_SINGLE, pm, f, 0, 1, &op)) return 1;
    const size_t nel = (size_t)(n1 + 2 * p1) * (n2 + 2 * p2);
    double *dx = nullptr, *dy = nullptr;
    int rc = 0;
    if (hipMalloc(reinterpret_cast<void**>(&dx), nel * sizeof(double)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dy), nel * sizeof(double)) != hipSuccess) {
        set_error("poms_kron_dot_2d: hipMalloc failed");
        rc = 1;
    }
    if (!rc && (hipMemcpy(dx, X, nel * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(dy, Y, nel * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)) {
        set_error("poms_kron_dot_2d: upload failed");
        rc = 1;
    }
    if (!rc) rc = poms_op_apply(op, dx, dy, 0, 1, nullptr);
    if (!rc && hipMemcpy(Y, dy, nel * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("poms_kron_dot_2d: download failed");
        rc = 1;
    }
    if (dx) (void)hipFree(dx);
    if (dy) (void)hipFree(dy);
    poms_op_destroy(op);
    return rc;
}

}  // extern "C"
