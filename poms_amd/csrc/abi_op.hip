// extern "C" boundary of libpoms_hip.so (declared in include/poms_hip.h): the error
// message, the context, and the operator object -- creation, variant selection, op_run
// with its wrappers and reductions, and launch timing.
#include "common.hpp"
#include "launchers.hpp"
#include "split_hooks.hpp"
#include "abi_internal.hpp"
#include "../../include/poms_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace poms {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
bool error_is_set() { return !g_err.empty(); }

int ctx_device(const poms_ctx* ctx) { return ctx->device; }

}  // namespace poms

using namespace poms;

// A launch-timing event; under stream capture it becomes an event-record node of the
// graph (every replay records it again), not a capture-ordering marker.
static hipError_t timing_record(hipEvent_t e, hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t q = hipStreamIsCapturing(s, &cs);
    if (q != hipSuccess) return q;
    if (cs != hipStreamCaptureStatusActive) return hipEventRecord(e, s);
    // an event-record node after the capture's current frontier, which it then replaces
    hipGraph_t g = nullptr;
    const hipGraphNode_t* deps = nullptr;
    size_t nd = 0;
    hipError_t r = hipStreamGetCaptureInfo_v2(s, &cs, nullptr, &g, &deps, &nd);
    if (r != hipSuccess) return r;
    hipGraphNode_t node = nullptr;
    r = hipGraphAddEventRecordNode(&node, g, deps, nd, e);
    if (r != hipSuccess) return r;
    return hipStreamUpdateCaptureDependencies(s, &node, 1, hipStreamSetCaptureDependencies);
}

static int resolve_variant(const poms_op* o, int epi);

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

// The per-axis quadrature tables on the device as ax[3]; an unused leading axis gets one
// element with one point of weight 1 and the constant function.  Every allocation goes
// onto `owned`, which the caller frees, also after a failure (returns 1).
static int upload_axes(int ndim, const int* nel, const int* nq, const int* p, const int* const* first,
                       const int* const* es, const int* const* ee, const double* const* basis,
                       const double* const* weights, const int64_t* nglob, AssembleAxis* ax,
                       std::vector<void*>& owned) {
    auto up = [&](const void* h, size_t bytes) -> void* {
        void* d = nullptr;
        if (hipMalloc(&d, std::max<size_t>(bytes, 8)) != hipSuccess) return nullptr;
        owned.push_back(d);
        if (hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    };
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

extern "C" {

int poms_abi_version(void) { return POMS_ABI_VERSION; }

const char* poms_last_error(void) { return g_err.c_str(); }

int poms_device_count(int* count) {
    if (!count) { set_error("null count"); return 1; }
    POMS_HIP_CHECK(hipGetDeviceCount(count));
    return 0;
}

int poms_ctx_create(int device, poms_ctx** ctx) {
    if (!ctx) { set_error("null ctx out"); return 1; }
    POMS_HIP_CHECK(hipSetDevice(device));
    auto* c = new poms_ctx();
    c->device = device;
    if (hipMalloc(reinterpret_cast<void**>(&c->scratch), kScratch * sizeof(double)) != hipSuccess) {
        delete c;
        set_error("hipMalloc scratch failed");
        return 1;
    }
    *ctx = c;
    return 0;
}

int poms_ctx_destroy(poms_ctx* ctx) {
    if (!ctx) return 0;
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    delete ctx;
    return 0;
}

int poms_synchronize(poms_ctx* ctx, void* stream) {
    (void)ctx;
    POMS_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
    return 0;
}

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

}  // extern "C"

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
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 1;
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
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 1;
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
    StencilGeom g{r.s0, r.s1, r.n0, r.n1, r.n2, r.pd0, r.pd1, r.pd2, o->sp[0], o->sp[1], o->sp[2],
                  2 * o->sp[0] + 1, 2 * o->sp[1] + 1, 2 * o->sp[2] + 1, (int64_t)r.n0 * r.n1 * r.n2, 0, 0, 0, 0};
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
    if (fine->g0 != 0 || (fine->ndim == 3 && fine->L.n[0] != fine->n0g) ||
        ((fine->L.flags | coarse_layout->flags) & POMS_LAYOUT_GHOST_DATA)) {
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
    auto dev = [&](const void* h, size_t bytes) -> void* {   // (h null: uninitialised)
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) return nullptr;
        tmp.push_back(p);
        if (h && hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return p;
    };
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
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 1;
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
                      o->spec_dev, o->spec_bak, o->la_raw})
        if (p) (void)hipFree(p);
    for (void* p : o->mf_tabs)
        if (p) (void)hipFree(p);
    if (o->mf_diag) (void)hipFree(o->mf_diag);
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

int poms_op_set_variant(poms_op* op, int variant) {
    // 90/91, 92-100, 101-113: diagnostic / tuning builds of v3, v4, v5 (110-112: v5
    // two sweeps from zero without sums / x1 scaling, timing only; 113: the Jacobi
    // sweep streaming the x rows no other tile reads)
    // (11, v7, was removed in round 6: an experimental kernel slower than v5)
    const bool known = variant == 0 || variant == 4 || (variant >= 7 && variant <= 10) ||
                       (variant >= 90 && variant <= 114);
    if (!op || !known) {
        set_error("poms_op_set_variant: bad argument (0, 4, 7, 8, 9, 10; 90-114 diagnostic)");
        return 1;
    }
    if (variant > 0 && !op->v2_ok) { set_error("poms_op_set_variant: variant needs pads == pmax"); return 1; }
    op->variant = variant;
    ++op->gen;
    return 0;
}

int poms_diag_v5_stamps(uint64_t* host_out, int64_t n) {
    if (!host_out) { set_error("poms_diag_v5_stamps: null argument"); return 1; }
    return kron_v5_stamps(reinterpret_cast<unsigned long long*>(host_out), n);
}

int poms_diag_v5_sched(int mode) { return kron_v5_set_sched(mode); }

int poms_variant_built(int variant) {
    return (variant == 0 || variant == 4 || (variant >= 7 && variant <= 10) || (variant >= 90 && variant <= 114)) ? 1 : 0;
}

int poms_op_kernel_variant(poms_op* op, int epilogue, int* variant) {
    if (!op || !variant || epilogue < EPI_APPLY || epilogue > EPI_APPLYDOT) {
        set_error("poms_op_kernel_variant: bad argument");
        return 1;
    }
    *variant = resolve_variant(op, epilogue);
    return 0;
}

int poms_op_last_variant(poms_op* op, int* variant) {
    if (!op || !variant) { set_error("poms_op_last_variant: null argument"); return 1; }
    *variant = op->last_variant;
    return 0;
}

int poms_op_spec_stats(poms_op* op, int* stats) {
    if (!op || !stats) { set_error("poms_op_spec_stats: null argument"); return 1; }
    stats[0] = op->spec_calls;
    stats[1] = op->spec_repeats;
    stats[2] = op->spec_graph_caps;
    stats[3] = op->spec_graph_hits;
    return 0;
}

// Dirichlet faces of a general form.  The mask is a run-time field of the launch
// geometry; bumping `gen` re-keys the captured graphs of poms_pcg_jacobi (nothing else the
// operator caches depends on what a launch computes).
int poms_op_set_dirichlet(poms_op* op, int faces) {
    const std::string fn = "poms_op_set_dirichlet: ";
    if (!op) { set_error(fn + "null argument"); return 1; }
    if (!general_form(op)) {
        set_error(fn + "Kronecker forms are constrained through their factors (needs a general-stencil or matrix-free operator)");
        return 1;
    }
    if (faces < 0 || faces >= (1 << (2 * op->ndim))) {
        set_error(fn + "faces has bits beyond 2 ndim = " + std::to_string(2 * op->ndim));
        return 1;
    }
    if (faces == 0 && op->dmask == 0) return 0;   // nothing to clear, on any layout
    if (op->g0 != 0 || (op->ndim == 3 && op->L.n[0] != op->n0g) || (op->L.flags & POMS_LAYOUT_GHOST_DATA)) {
        set_error(fn + "distributed operators (slabs, Cart blocks) are not supported");
        return 1;
    }
    // (the legacy stream answers for a capture in progress on any stream of the thread
    // in the global capture mode; the operator's own capture stream is asked as well)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    bool capturing = hipStreamIsCapturing(nullptr, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    if (!capturing && op->cap_stream)
        capturing = hipStreamIsCapturing(op->cap_stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    if (capturing) {
        (void)hipGetLastError();
        set_error(fn + "called during a stream capture");
        return 1;
    }
    const int m = faces << (2 * (3 - op->ndim));   // the operator's axes are the kernels' last ndim
    if (m == op->dmask) return 0;
    op->dmask = m;
    op->mf_geom.dmask = m;
    ++op->gen;
    return 0;
}

int poms_op_get_dirichlet(poms_op* op, int* faces) {
    if (!op || !faces) { set_error("poms_op_get_dirichlet: null argument"); return 1; }
    *faces = op->dmask >> (2 * (3 - op->ndim));
    return 0;
}

int poms_op_get_variant(poms_op* op, int* variant) {
    if (!op || !variant) { set_error("poms_op_get_variant: null argument"); return 1; }
    *variant = op->variant;
    return 0;
}

int poms_op_set_tile_cols(poms_op* op, int cols) {
    if (!op || cols < 0 || cols > 64 - 2 * op->pmax) { set_error("poms_op_set_tile_cols: bad argument"); return 1; }
    op->tout = cols;
    ++op->gen;
    return 0;
}

int poms_op_set_chunk(poms_op* op, int chunk) {
    if (!op || chunk < 0) { set_error("poms_op_set_chunk: bad argument"); return 1; }
    op->chunk = chunk;
    ++op->gen;
    return 0;
}

// Axis-0 chunk length.  A workgroup streams `chunk` planes plus 2p halo planes, so
// long chunks save re-reads but leave a ragged last round of workgroups on the
// 256 CUs (512 resident workgroups at p <= 3).  Cost of nc chunks ~ rounds(nc) *
// (chunk + 2p), the partial last round weighted 5x its fill (fit to the chunk sweeps
// in profiles/r01/chunks/*.log; picks 103 at 515^3 p=3, 43 at 258^3 p=2).  For
// p >= 4 the kernels are VALU-bound and want >= 3 workgroups per CU instead.
static int auto_chunk(int nz, int tiles, int p, double slots = 512.0) {
    if (nz <= 0) return 1;
    tiles = std::max(tiles, 1);
    if (p >= 4 && slots > 256.0) {
        const int nc = std::max(1, std::min(nz / 8, (768 + tiles - 1) / tiles));
        return (nz + nc - 1) / nc;
    }
    double best = 1e300;
    int best_chunk = nz;
    for (int nc = 1; nc <= std::max(1, nz / 8); ++nc) {
        const int ch = (nz + nc - 1) / nc;
        const double r = (double)nc * tiles / slots;
        const double fr = std::floor(r);
        const double rounds = r > 1.0 ? fr + std::min(1.0, (r - fr) * 5.0) : 1.0;
        const double cost = rounds * (ch + 2 * p);
        if (cost < best - 1e-9) { best = cost; best_chunk = ch; }
    }
    return best_chunk;
}

// v5 (variant 10) runs 3D FORM_SUM operators, p <= 3, pads == pmax, arrays < 2 GiB.
// At odd p its x-row DMA pairs straddle storage column 0, and the pair holding
// column 0 of storage row 0 (the corner ghost of each plane) fails the buffer range
// check: zero, as the ghost always is unless axes 1 and 2 both have a lower
// neighbour -- then (ghost_corners) the operator runs v3.
static bool v5_ok(const poms_op* o) {
    const int64_t bytes = (int64_t)(o->L.n[0] + 2 * o->L.pads[0]) * row_geom(&o->L).s0 * 8;
    return o->ndim == 3 && o->form == FORM_SUM && o->v2_ok && o->pmax <= 5 && bytes < 0x7ffffff0LL &&
           !(o->ghost_corners && (o->pmax & 1));
}

// v5 tiles are line-aligned when the row pitch is a multiple of 16 doubles and
// interior column 0 of x starts a 128-B line
static bool v5_aligned(const poms_op* o, const double* x) {
    const int64_t pitch = row_geom(&o->L).s1;
    return pitch % 16 == 0 && (reinterpret_cast<uintptr_t>(x + o->L.pads[2]) & 127) == 0;
}

static bool same_toeplitz12(const poms_op* o);

static int op_geom(poms_op* o, int64_t zb, int64_t ze, KronGeom& g, int v = -1, int v5_to = 0,
                   int64_t zb2 = 0, int64_t ze2 = 0, int epi = EPI_APPLY) {
    if (v < 0) v = o->variant;
    const bool is3d = o->ndim == 3;
    const RowGeom r = row_geom(&o->L);
    g.s0 = r.s0;
    g.s1 = r.s1;
    g.n0 = r.n0; g.n1 = r.n1; g.n2 = r.n2;
    g.pd0 = r.pd0; g.pd1 = r.pd1; g.pd2 = r.pd2;
    g.g0 = (int)o->g0;
    g.tiles2 = (int)((o->L.n[2] + kron_tile_cols() - 1) / kron_tile_cols());
    const int trows = v == 10 ? kron_v5_rows(o->pmax, epi, same_toeplitz12(o) ? 1 : 0)
                    : (!is3d && v == 9 && o->pmax == 3) ? kron_v3_rows_2d() : kron_tile_rows();
    g.tiles1 = (int)((o->L.n[1] + trows - 1) / trows);
    g.tout = v == 10 ? v5_to : (o->tout > 0 ? o->tout : 64 - 2 * o->pmax);
    if (v >= 4) g.tiles2 = (int)((o->L.n[2] + g.tout - 1) / g.tout);
    if (!is3d) {
        g.z_begin = 0; g.z_end = 1; g.chunk = 1; g.nchunks = 1; g.nch1 = 1; g.z2_begin = g.z2_end = 0;
        return 0;
    }
    if (zb < 0 || ze > o->L.n[0] || zb > ze) { set_error("plane range outside the slab"); return 1; }
    if (zb2 < 0 || ze2 > o->L.n[0] || zb2 > ze2 || (ze2 > zb2 && zb2 < ze && ze2 > zb)) {
        set_error("second plane range outside the slab or overlapping the first");
        return 1;
    }
    {   // tile order (tuning: POMS_TILE_ORDER=0/1)
        static int ord = -1;
        if (ord < 0) {
            const char* e = getenv("POMS_TILE_ORDER");
            ord = e ? (atoi(e) ? 1 : 0) : 0;
        }
        g.order = ord;
    }
    g.z_begin = (int)zb;
    g.z_end = (int)ze;
    g.z2_begin = (int)zb2;
    g.z2_end = (int)ze2;
    const int nz = (int)(ze - zb) + (int)(ze2 - zb2);
    int chunk = o->chunk;
    if (chunk <= 0) {
        const double slots = v == 10 ? 256.0 : 512.0;
        const int tiles = g.tiles2 * g.tiles1;
        chunk = auto_chunk(nz, tiles, o->pmax, slots);
        // The interior launch of a distributed call shares the GPU with the exchange and
        // the boundary launch on the communication stream: one chunk (one short round
        // that leaves CUs to them) where it fits 3/4 of the slots and costs at most 1.4x
        // the plane steps of the chunked grid (POMS_SPLIT_ONE=0: off).  Loopback proxy,
        // rank 1, interleaved (profiles/r06/split_chunk/): 8 ranks (59 interior planes)
        // 41.7-41.8 -> 38.7-38.9 ms per cycle, 4 ranks (123) 60.6-60.8 -> 58.8-59.1 ms;
        // at 2 ranks (252 planes, 1.43x) one chunk was slower (103.7 -> 111.1 ms) and
        // the rule keeps the chunks there
        static const bool split_one = !(getenv("POMS_SPLIT_ONE") && getenv("POMS_SPLIT_ONE")[0] == '0');
        bool one = false;
        if (o->split_interior && split_one && tiles <= 0.75 * slots && chunk < nz) {
            const int nc = (nz + chunk - 1) / chunk;
            const double r = (double)nc * tiles / slots;
            const double fr = std::floor(r);
            const double rounds = r > 1.0 ? fr + std::min(1.0, (r - fr) * 5.0) : 1.0;
            one = nz + 2 * o->pmax <= 1.4 * rounds * (chunk + 2 * o->pmax);
            if (one) chunk = nz;
        }
        // the v5 two-sweeps-from-zero launch (VALU-bound) balances better over twice
        // as many chunks: 515^3 p = 3, 86 instead of 172 planes, 836-838 against
        // 865-882 us in two interleaved sweeps, equal medians (833 us) in a third
        // (profiles/r03/chunks/); the other epilogues keep the model's pick (Jacobi
        // 715 us at 172 against 729 at 86)
        if (!one && v == 10 && epi == EPI_JACOBI0 && o->pmax == 3 && same_toeplitz12(o) && chunk / 2 >= 8 * o->pmax)
            chunk = (chunk + 1) / 2;   // (the 16-wave build only)
    }
    chunk = std::max(1, std::min(chunk, std::max(nz, 1)));
    g.chunk = chunk;
    g.nch1 = (int)((ze - zb + chunk - 1) / chunk);
    g.nchunks = g.nch1 + (int)((ze2 - zb2 + chunk - 1) / chunk);
    return 0;
}

// variants whose Jacobi epilogue also accumulates x_out . b (v3 and v4 kernels)
static bool fused_dot_ok(const poms_op* o) {
    return general_form(o) || (o->variant >= 4 && o->variant <= 10) || o->variant == 114;
}


// General-stencil launch (FORM_STENCIL): the epilogues of op_run plus EPI_DIAG.
static int stencil_run(poms_op* o, int epi, double omega, const double* x, double* y, const double* b,
                       int64_t zb, int64_t ze, int want_norm, void* stream, int want_dot, int64_t zb2,
                       int64_t ze2, PartRoute* route = nullptr, double beta = 0.0) {
    if (route) route->used = false;   // (its own partials layout: the scratch only)
    if (epi == EPI_JACOBI0) { set_error("general stencil: no two-sweeps-from-zero epilogue"); return 1; }
    if (want_dot && epi != EPI_JACOBI && epi != EPI_APPLYDOT) { set_error("general stencil: dot needs Jacobi / apply+dot"); return 1; }
    const RowGeom r = row_geom(&o->L);
    if (zb < 0 || ze > r.n0 || zb > ze || zb2 < 0 || ze2 > r.n0 || zb2 > ze2) { set_error("general stencil: bad plane range"); return 1; }
    StencilGeom g{r.s0, r.s1, r.n0, r.n1, r.n2, r.pd0, r.pd1, r.pd2, o->sp[0], o->sp[1], o->sp[2],
                  2 * o->sp[0] + 1, 2 * o->sp[1] + 1, 2 * o->sp[2] + 1, (int64_t)r.n0 * r.n1 * r.n2,
                  (int)zb, (int)ze, (int)zb2, (int)ze2, o->dmask};
    const int maxb = (int)(kScratch / 2);
    int nb = 0;
    double* scr = o->ctx->scratch;
    const bool red = want_norm || want_dot || epi == EPI_APPLYDOT;
    if (stencil_launch(epi, g, o->coef, x, y, b, omega, want_norm ? scr : nullptr,
                       (want_dot || epi == EPI_APPLYDOT) ? scr + std::min<int64_t>(maxb, std::max<int64_t>(1, ((int64_t)(ze - zb + ze2 - zb2) * r.n1 * r.n2 + 255) / 256)) : nullptr,
                       maxb, as_stream(stream), &nb, beta))
        return 1;
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = red ? nb : 0;
    return 0;
}

// Matrix-free launch (FORM_MATFREE): stencil_run's epilogues and partials layout
// (norms at scratch[0, nb), dots behind them).  The whole grid in one launch: the
// operator is undistributed, so the plane range must be all of axis 0.  Nothing is
// allocated or synchronised here.
static int matfree_run(poms_op* o, int epi, double omega, const double* x, double* y, const double* b,
                       int64_t zb, int64_t ze, int want_norm, void* stream, int want_dot, int64_t zb2,
                       int64_t ze2, PartRoute* route = nullptr, double beta = 0.0) {
    if (route) route->used = false;   // (stencil_run's layout: the scratch only)
    if (epi == EPI_JACOBI0) { set_error("matrix-free operator: no two-sweeps-from-zero epilogue"); return 1; }
    if (want_dot && epi != EPI_JACOBI && epi != EPI_APPLYDOT) { set_error("matrix-free operator: dot needs Jacobi / apply+dot"); return 1; }
    const RowGeom r = row_geom(&o->L);
    if (zb != 0 || ze != r.n0 || zb2 != ze2) { set_error("matrix-free operator: the plane range must be the whole axis 0"); return 1; }
    const int maxb = (int)(kScratch / 2);
    double* scr = o->ctx->scratch;
    int nb = 0;
    if (epi == EPI_DIAG) {   // x = scale b / diag: the general stencil's kernel on the stored diagonal
        StencilGeom g{r.s0, r.s1, r.n0, r.n1, r.n2, r.pd0, r.pd1, r.pd2, 0, 0, 0, 1, 1, 1,
                      (int64_t)r.n0 * r.n1 * r.n2, 0, r.n0, 0, 0};
        if (stencil_launch(EPI_DIAG, g, o->mf_diag, x, y, b, omega, want_norm ? scr : nullptr, nullptr, maxb,
                           as_stream(stream), &nb))
            return 1;
        POMS_HIP_CHECK(hipGetLastError());
        o->last_partials = want_norm ? nb : 0;
        return 0;
    }
    if ((epi == EPI_JACOBI || epi == EPI_APPLYDOT || epi == EPI_CHEBY) && x == y) { set_error("matrix-free operator: y must not alias x"); return 1; }
    const MatfreeGeom& g = o->mf_geom;
    const int nblk = (int)std::min<int64_t>(g.ntiles, maxb);
    const bool wd = want_dot || epi == EPI_APPLYDOT;
    if (matfree_launch(epi, g, o->mf_ax, x, y, b, o->mf_a, o->mf_c, o->mf_diag, o->mf_mass, omega,
                       want_norm ? scr : nullptr, wd ? scr + nblk : nullptr, maxb, as_stream(stream), &nb,
                       o->mf_tensor, beta))
        return 1;
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = (want_norm || wd) ? nb : 0;
    return 0;
}

// axis 1 and axis 2 share their Toeplitz rows bitwise (v5's SAME12 builds)
static bool same_toeplitz12(const poms_op* o) {
    for (int k = 0; k <= o->pmax; ++k)
        if (o->tc.t1a[k] != o->tc.t2a[k] || o->tc.t1b[k] != o->tc.t2b[k]) return false;
    return true;
}

// 2D Jacobi sweeps at p <= 3: v3 (9) by default; POMS_JAC2D_VARIANT=7 selects v4
// (tuning knob)
static int jacobi2d_variant() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("POMS_JAC2D_VARIANT");
        v = (e && atoi(e) == 7) ? 7 : 9;
    }
    return v;
}

// The kernel variant one launch of epilogue `epi` runs (see op_run).
static int resolve_variant(const poms_op* o, int epi) {
    int v = o->variant;
    if (v == 8) {
        const bool plain = epi == EPI_APPLY || epi == EPI_RESID || epi == EPI_JACOBI;
        if (o->ndim == 3 && v5_ok(o))
            v = 10;   // v5: kernel_bench at 515^3 p = 3; 8-wave tiles at 256^3 p = 4, 5
                      // (profiles/r02/configs/kb_p5_waves8.log: apply 231 -> 185 us at p = 5);
                      // sweeps from zero at p <= 2 and p = 4, 5 (8-wave tiles; at 256^3
                      // p = 4 208 vs 291 us for v3, p = 5 261 vs 428 us,
                      // profiles/r05/late/kb_p45_j0.log) and at p = 3 (16-wave tiles, 930 vs
                      // 945 us for v3 at 515^3, profiles/r02/j0_16wave/) where axes 1 and 2
                      // share their rows, 8-wave tiles where they do not (round 6; the
                      // 16-wave build of that case spills)
        else if (o->ndim == 3)
            v = ((epi == EPI_APPLY && o->pmax >= 3) || (plain && o->pmax >= 4)) ? 7 : 9;
        else if (epi == EPI_JACOBI && o->pmax <= 3)
            v = jacobi2d_variant();
        else
            v = ((epi == EPI_APPLY || epi == EPI_RESID) && o->pmax <= 3) ? 7 : 9;
    }
    if (v == 10 && !v5_ok(o)) v = 9;
    return v;
}

}  // extern "C"

// Two Jacobi sweeps per launch (EPI_JACOBI2, kron_2d.hip): one-rank 2D p = 3
// Kronecker operators whose single sweep runs the v3 whole-array kernel (variant 9),
// whose bits the two-sweep kernel reproduces
bool poms::sweep2_ok(const poms_op* o) {
    if (o->ndim != 2 || o->pmax != 3 || general_form(o) || o->ghost_corners) return false;
    if (o->L.pads[1] != 3 || o->L.pads[2] != 3 || resolve_variant(o, EPI_JACOBI) != 9) return false;
    return padded_len(o) * 8 < 0x7ffffff0LL;
}

extern "C" {

// Where a launch of nblk blocks writes its partials (none wanted: null pointers): the
// route's destination when its sums fit there (route->used), norms at *pn and dots behind
// them at *pd; else the scratch, norms at part_off and dots at dot_base (default nblk) +
// part_off.  The scratch must hold them even when the route takes them.  `three`
// (EPI_JACOBI3Z): three sums side by side from *pn, which the scratch holds only in its
// default layout and need not hold when the route takes them.
static int part_place(poms_op* o, int64_t nblk, bool wn, bool wd, bool three, PartRoute* route, double** pn,
                      double** pd) {
    if (route) route->used = false;
    *pn = *pd = nullptr;
    if (!wn && !wd) return 0;
    const int64_t dbase = o->dot_base < 0 ? nblk : o->dot_base;
    const bool fits = three ? o->part_off == 0 && o->dot_base < 0 && 3 * nblk <= kScratch
                            : o->part_off + nblk <= dbase && dbase + o->part_off + nblk <= kScratch;
    const bool sink = route && route->dst && (three ? 3 : (wn ? 1 : 0) + (wd ? 1 : 0)) * nblk <= route->cap;
    if (!fits && !(three && sink)) { set_error("too many blocks for the partial-sum scratch"); return 1; }
    *pn = sink ? route->dst : o->ctx->scratch + o->part_off;
    *pd = sink ? route->dst + (wn ? nblk : 0) : o->ctx->scratch + dbase + o->part_off;
    if (sink) route->used = true;
    return 0;
}

// partials as op_run: norm (sweep k+1) and dot (sweep k) at the route's destination / the
// scratch.  EPI_JACOBI3Z (x = b): all three sums or none, ||x1||^2, ||dr_2||^2, ||dr_3||^2
// side by side (the route's destination, or scratch[0, 3n))
static int op_run_j2(poms_op* o, int epi, double omega, const double* x, double* y, const double* b, int want_norm,
                     int want_dot, void* stream, PartRoute* route) {
    if (!sweep2_ok(o)) { set_error("two sweeps per launch: one-rank 2D p = 3 Kronecker operators (variant 9) only"); return 1; }
    if (x == y || b == y) { set_error("two sweeps per launch: x_out must not alias x_in or b"); return 1; }
    const bool fz = epi == EPI_JACOBI3Z;
    if (fz && (x != b || want_norm != want_dot)) { set_error("three sweeps from zero: x = b, all three sums or none"); return 1; }
    KronGeom g;
    if (op_geom(o, 0, 1, g, 9, 0, 0, 0, EPI_JACOBI)) return 1;
    const int trows = fz ? kron2d_j2_rows_default() : kron2d_j2_rows();
    g.tout = kron2d_j2_cols(o->pmax);
    g.tiles2 = (int)((o->L.n[2] + g.tout - 1) / g.tout);
    g.tiles1 = (int)((o->L.n[1] + trows - 1) / trows);
    const int64_t nblk = (int64_t)g.tiles2 * g.tiles1;
    o->last_variant = 9;
    if (nblk == 0) { o->last_partials = 0; return 0; }
    double *pn = nullptr, *pd = nullptr;
    if (part_place(o, nblk, want_norm, want_dot, fz, route, &pn, &pd)) return 1;
    if (fz) {   // (pn: the three sums' base, pd = pn + nblk)
        KronPtrs p{b, y, b, o->a0t, o->b0t, o->a1, o->b1, o->a2, o->b2, pn ? pn + 2 * nblk : nullptr, pd, nullptr};
        if (kron2d_j2_launch(o->pmax, o->form, p, g, o->tc, omega, as_stream(stream), true, pn)) return 1;
        POMS_HIP_CHECK(hipGetLastError());
        o->last_partials = want_norm ? nblk : 0;
        return 0;
    }
    KronPtrs p{x, y, b, o->a0t, o->b0t, o->a1, o->b1, o->a2, o->b2, want_norm ? pn : nullptr,
               want_dot ? pd : nullptr, nullptr};
    if (kron2d_j2_launch(o->pmax, o->form, p, g, o->tc, omega, as_stream(stream), false, nullptr)) return 1;
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = (want_norm || want_dot) ? nblk : 0;
    return 0;
}

static int op_run(poms_op* o, int epi, double omega, const double* x, double* y, const double* b,
                  int64_t zb, int64_t ze, int want_norm, void* stream, int want_dot = 0,
                  int64_t zb2 = 0, int64_t ze2 = 0, PartRoute* route = nullptr, double beta = 0.0) {
    if (!o || !x || !y) { set_error("null operator or vector"); return 1; }
    if (epi != EPI_APPLY && !b) { set_error("null right-hand side"); return 1; }
    if (epi == EPI_JACOBI2 || epi == EPI_JACOBI3Z)
        return op_run_j2(o, epi, omega, x, y, b, want_norm, want_dot, stream, route);
    if (o->form == FORM_STENCIL)
        return stencil_run(o, epi, omega, x, y, b, zb, ze, want_norm, stream, want_dot, zb2, ze2, route, beta);
    if (o->form == FORM_MATFREE)
        return matfree_run(o, epi, omega, x, y, b, zb, ze, want_norm, stream, want_dot, zb2, ze2, route, beta);
    if (epi == EPI_CHEBY) { set_error("Chebyshev step: general-stencil and matrix-free operators only"); return 1; }
    if (epi == EPI_APPLYDOT && !(o->variant == 4 || o->variant == 8 || o->variant == 9 || o->variant == 10)) {
        set_error("apply + x.y: kernel variants 4, 8, 9, 10 only");
        return 1;
    }
    if (want_dot && ((epi != EPI_JACOBI && epi != EPI_JACOBI0 && epi != EPI_APPLYDOT) || !fused_dot_ok(o))) {
        set_error("fused x_out.b needs a Jacobi sweep on kernel variants 4-10");
        return 1;
    }
    if (epi == EPI_JACOBI0 && !(o->variant == 8 || o->variant == 9 || o->variant == 10 ||
                                (o->variant >= 110 && o->variant <= 112) || o->variant == 114)) {
        set_error("two sweeps from zero: kernel variant 8, 9 or 10 only");
        return 1;
    }
    // variant 8 (default when pads == pmax): the fastest measured kernel per
    // epilogue (profiles/r01/chunks/*.log) -- in 3D v4 (7) for apply at p >= 3 and
    // for every plain epilogue at p >= 4 (VALU-bound there), v3 with whole-array
    // buffer resources (9; falls back to 4 for arrays >= 2 GiB) otherwise; in 2D
    // v4 for apply / residual at p <= 3.  Fused dots and two-sweeps-from-zero: 9.
    // Variant 10 (v5) runs apply / residual / Jacobi / apply+dot of 3D p <= 3
    // operators, and is what 8 picks for them; 9 otherwise.
    int v = resolve_variant(o, epi);
    const int v5_diag = (v >= 101 && v <= 114) ? v - 100 : 0;   // v5 diagnostic / tuning builds
    if (v5_diag) v = 10;
    o->last_variant = v5_diag ? 100 + v5_diag : v;
    int v5_h = 0, v5_to = 0;
    if (v == 10) kron_v5_tile(o->pmax, v5_aligned(o, x), &v5_h, &v5_to);
    KronGeom g;
    if (op_geom(o, zb, ze, g, v, v5_to, zb2, ze2, epi)) return 1;
    const int64_t nblk = (int64_t)g.tiles2 * g.tiles1 * g.nchunks;
    if (nblk == 0) { o->last_partials = 0; return 0; }
    double *pn = nullptr, *pd = nullptr;
    if (part_place(o, nblk, want_norm, want_dot, false, route, &pn, &pd)) return 1;
    KronPtrs p{x, y, b, o->a0t, o->b0t, o->a1, o->b1, o->a2, o->b2, want_norm ? pn : nullptr,
               want_dot ? pd : nullptr, o->rdiag0};
    poms_op::TimedLaunch* tlh = nullptr;
    bool tl_ext = false;
    if (o->timing && (o->t_epi < 0 || o->t_epi == epi) && (o->t_seen++ % o->t_every) == 0) {
        // events on the launch stream around this launch (a sample: every t_every-th)
        if (o->tl_used == o->tl.size()) {
            poms_op::TimedLaunch t{};
            POMS_HIP_CHECK(hipEventCreate(&t.e0));
            POMS_HIP_CHECK(hipEventCreate(&t.e1));
            o->tl.push_back(t);
        }
        tlh = &o->tl[o->tl_used++];
        tlh->epi = epi;
        tlh->ndof = (int64_t)((ze - zb) + (ze2 - zb2)) * g.n1 * g.n2;
        // v5 outside a capture: the events ride on the kernel's own dispatch
        // (hipExtLaunchKernel start / stop), i.e. the kernel's execution time as
        // rocprofv3 reports it; otherwise event records before and after the launch
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        POMS_HIP_CHECK(hipStreamIsCapturing(as_stream(stream), &cs));
        if (v == 10 && cs == hipStreamCaptureStatusNone) {
            kron_v5_set_launch_events(tlh->e0, tlh->e1);
            tl_ext = true;
        } else {
            POMS_HIP_CHECK(timing_record(tlh->e0, as_stream(stream)));
        }
    }
    const int rc = v == 10
        ? kron_v5_launch(o->pmax, epi, p, g, o->tc, v5_h, omega, as_stream(stream), v5_diag)
        : v == 0
        ? kron_launch(o->pmax, o->ndim == 3, o->form, epi, p, g, omega, as_stream(stream))
        : (v == 7 || (v >= 92 && v <= 100))
        ? kron_v4_launch(o->pmax, o->ndim == 3, o->form, epi, p, g, o->tc, omega, as_stream(stream),
                         v == 7 ? 0 : v - 91)
        : kron_v3_launch(v, o->pmax, o->ndim == 3, o->form, epi, p, g, o->tc, omega, as_stream(stream));
    if (tl_ext && !kron_v5_launch_events_used()) {   // (the v5 launch failed before its dispatch)
        kron_v5_set_launch_events(nullptr, nullptr);
        if (!rc) { set_error("v5: timed launch did not take its events"); return 1; }
    }
    if (tlh && !tl_ext) POMS_HIP_CHECK(timing_record(tlh->e1, as_stream(stream)));
    if (rc) return 1;
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = (want_norm || want_dot) ? nblk : 0;
    return 0;
}

int poms_op_apply(poms_op* op, const double* x, double* y, int64_t zb, int64_t ze, void* stream) {
    return op_run(op, EPI_APPLY, 0.0, x, y, nullptr, zb, ze, 0, stream);
}

int poms_op_residual(poms_op* op, const double* b, const double* x, double* r, int64_t zb,
                     int64_t ze, void* stream) {
    return op_run(op, EPI_RESID, 0.0, x, r, b, zb, ze, 0, stream);
}

int poms_op_jacobi_sweep(poms_op* op, double omega, const double* b, const double* x_in,
                         double* x_out, int64_t zb, int64_t ze, int want_norm, void* stream) {
    if (x_in == x_out) { set_error("jacobi sweep: x_out must not alias x_in"); return 1; }
    return op_run(op, EPI_JACOBI, omega, x_in, x_out, b, zb, ze, want_norm, stream);
}

int poms_op_jacobi_sweep_dot(poms_op* op, double omega, const double* b, const double* x_in,
                             double* x_out, int64_t zb, int64_t ze, int want_norm, void* stream) {
    if (x_in == x_out) { set_error("jacobi sweep: x_out must not alias x_in"); return 1; }
    return op_run(op, EPI_JACOBI, omega, x_in, x_out, b, zb, ze, want_norm, stream, 1);
}

int poms_op_apply_dot(poms_op* op, const double* x, double* y, int64_t zb, int64_t ze, void* stream) {
    if (x == y) { set_error("apply: y must not alias x"); return 1; }
    return op_run(op, EPI_APPLYDOT, 0.0, x, y, x, zb, ze, 0, stream, 1);
}

// the forms and layouts whose Chebyshev step is one launch: the general forms, undistributed
static bool cheby_ok(const poms_op* o) {
    return general_form(o) && o->g0 == 0 && !(o->ndim == 3 && o->L.n[0] != o->n0g) &&
           !(o->L.flags & POMS_LAYOUT_GHOST_DATA);
}

int poms_op_cheby_step(poms_op* op, double alpha, double beta, const double* b, const double* x, double* y,
                       int64_t zb, int64_t ze, void* stream) {
    const std::string fn = "poms_op_cheby_step: ";
    if (!op || !b || !x || !y) { set_error(fn + "null argument"); return 1; }
    if (y == x || y == b) { set_error(fn + "y must not alias x or b"); return 1; }
    if (!general_form(op)) {
        set_error(fn + "Kronecker forms have no fused step (compose poms_op_jacobi_sweep and poms_vec_axpby)");
        return 1;
    }
    if (!cheby_ok(op)) { set_error(fn + "distributed operators (slabs, Cart blocks) are not supported"); return 1; }
    return op_run(op, EPI_CHEBY, alpha, x, y, b, zb, ze, 0, stream, 0, 0, 0, nullptr, beta);
}

int poms_op_cheby_supported(poms_op* op, int* yes) {
    if (!op || !yes) { set_error("poms_op_cheby_supported: null argument"); return 1; }
    *yes = cheby_ok(op) ? 1 : 0;
    return 0;
}

int poms_op_apply_dot_supported(poms_op* op, int* yes) {
    if (!op || !yes) { set_error("poms_op_apply_dot_supported: null argument"); return 1; }
    const int v = op->variant;
    *yes = (general_form(op) || v == 4 || v == 8 || v == 9 || v == 10) ? 1 : 0;
    return 0;
}

int poms_op_jacobi_from_zero(poms_op* op, double omega, const double* b, double* x_out,
                             int64_t zb, int64_t ze, int want_norm, void* stream) {
    if (!op || !b || !x_out) { set_error("jacobi from zero: null argument"); return 1; }
    if (b == x_out) { set_error("jacobi from zero: x_out must not alias b"); return 1; }
    int yes = 0;
    if (poms_op_from_zero_supported(op, &yes)) return 1;
    if (!yes) { set_error("jacobi from zero: not supported by this operator (poms_op_from_zero_supported)"); return 1; }
    return op_run(op, EPI_JACOBI0, omega, b, x_out, b, zb, ze, want_norm, stream, want_norm);
}

int poms_op_from_zero_supported(poms_op* op, int* yes) {
    if (!op || !yes) { set_error("poms_op_from_zero_supported: null argument"); return 1; }
    const int64_t bytes = padded_len(op) * 8;
    // 2D (round 6, v3): not on a block of a decomposition (its ghost rows' x1 would need
    // the neighbours' diagonal)
    *yes = ((op->ndim == 3 || (op->ndim == 2 && !op->ghost_corners)) && !general_form(op) &&
            (op->variant == 8 || op->variant == 9 || op->variant == 10 ||
             (op->variant >= 110 && op->variant <= 112) || op->variant == 114) &&
            bytes < 0x7ffffff0LL) ? 1 : 0;
    return 0;
}

int poms_op_sweep2_supported(poms_op* op, int* yes) {
    if (!op || !yes) { set_error("poms_op_sweep2_supported: null argument"); return 1; }
    *yes = sweep2_ok(op) ? 1 : 0;
    return 0;
}

int poms_op_jacobi3_from_zero(poms_op* op, double omega, const double* b, double* x_out, double* norms_out,
                              void* stream) {
    if (!op || !b || !x_out) { set_error("jacobi3 from zero: null argument"); return 1; }
    const bool wn = norms_out != nullptr;
    if (op_run(op, EPI_JACOBI3Z, omega, b, x_out, b, 0, 1, wn ? 1 : 0, stream, wn ? 1 : 0)) return 1;
    const int64_t n = op->last_partials;
    if (wn)
        for (int i = 0; i < 3; ++i)
            if (reduce_launch(op->ctx->scratch + i * n, (int)n, norms_out + i, as_stream(stream))) {
                set_error("jacobi3 from zero: reduction launch failed");
                return 1;
            }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_op_fused_dot_supported(poms_op* op, int* yes) {
    if (!op || !yes) { set_error("poms_op_fused_dot_supported: null argument"); return 1; }
    *yes = fused_dot_ok(op) ? 1 : 0;
    return 0;
}

int poms_op_diag_scale(poms_op* o, double scale, const double* b, double* x, int want_norm,
                       void* stream) {
    if (!o || !b || !x) { set_error("poms_op_diag_scale: null argument"); return 1; }
    if (o->form == FORM_STENCIL)
        return stencil_run(o, EPI_DIAG, scale, b, x, b, 0, o->L.n[0], want_norm, stream, 0, 0, 0);
    if (o->form == FORM_MATFREE)
        return matfree_run(o, EPI_DIAG, scale, b, x, b, 0, o->L.n[0], want_norm, stream, 0, 0, 0);
    const RowGeom g = row_geom(&o->L);
    int nb = 0;
    diag_scale_launch(o->ndim == 3, o->form, g, o->pmax, (int)o->g0, scale, b, x, o->a0t, o->b0t,
                      o->a1, o->b1, o->dg2a, o->dg2b, want_norm ? o->ctx->scratch : nullptr,
                      as_stream(stream), &nb);
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = want_norm ? nb : 0;
    return 0;
}

int poms_op_set_ghost_corners(poms_op* op, int yes) {
    if (!op) { set_error("poms_op_set_ghost_corners: null operator"); return 1; }
    op->ghost_corners = yes != 0;
    ++op->gen;
    return 0;
}

// One launch plus its reductions (one host call instead of three); the launch
// may cover a second plane range [zb2, ze2) (the slab's other boundary).
}  // extern "C"

// One launch of `epilogue` over planes [zb, ze) + [zb2, ze2), its partials written to
// the route's destination where one is given and they fit, else where op->part_off /
// dot_base say (part_place); the argument checks of poms_op_run_reduce2.
int poms::op_run_epi(poms_op* op, int epilogue, double omega, const double* x, double* y, const double* b,
                     int64_t zb, int64_t ze, int64_t zb2, int64_t ze2, bool wn, bool wd, void* stream,
                     PartRoute* route) {
    switch (epilogue) {
        case EPI_APPLY:
            if (wn || wd) { set_error("poms_op_run_reduce: apply has no reductions"); return 1; }
            if (op_run(op, EPI_APPLY, 0.0, x, y, nullptr, zb, ze, 0, stream, 0, zb2, ze2)) return 1;
            break;
        case EPI_RESID:
            if (wn || wd) { set_error("poms_op_run_reduce: residual has no reductions"); return 1; }
            if (op_run(op, EPI_RESID, 0.0, x, y, b, zb, ze, 0, stream, 0, zb2, ze2)) return 1;
            break;
        case EPI_JACOBI:
            if (x == y) { set_error("jacobi sweep: x_out must not alias x_in"); return 1; }
            if (op_run(op, EPI_JACOBI, omega, x, y, b, zb, ze, wn ? 1 : 0, stream, wd ? 1 : 0, zb2, ze2, route)) return 1;
            break;
        case EPI_JACOBI0:   // x = b: norm_out <- ||dr_2||^2, dot_out <- ||x1||^2
            {
                int fz = 0;
                if (poms_op_from_zero_supported(op, &fz)) return 1;
                if (!fz) { set_error("jacobi from zero: not supported by this operator"); return 1; }
            }
            if (b == y) { set_error("jacobi from zero: x_out must not alias b"); return 1; }
            if (wn != wd) { set_error("jacobi from zero: both norms or neither"); return 1; }
            if (op_run(op, EPI_JACOBI0, omega, b, y, b, zb, ze, wn ? 1 : 0, stream, wn ? 1 : 0, zb2, ze2, route)) return 1;
            break;
        case EPI_JACOBI2:   // two sweeps from x: norm_out <- ||dr_{k+1}||^2, dot_out <- ||dr_k||^2
            if (zb != 0 || ze != 1 || zb2 != ze2) { set_error("two sweeps per launch: 2D (planes [0, 1))"); return 1; }
            if (op_run(op, EPI_JACOBI2, omega, x, y, b, 0, 1, wn ? 1 : 0, stream, wd ? 1 : 0, 0, 0, route)) return 1;
            break;
        case EPI_JACOBI3Z:   // sweeps 1-3 from x = 0 (x = b): norm_out <- ||dr_3||^2, dot_out <- ||dr_2||^2
            // (poms_op_run_reduce2 cannot return the third sum: poms_op_jacobi3_from_zero)
            if (zb != 0 || ze != 1 || zb2 != ze2) { set_error("three sweeps from zero: 2D (planes [0, 1))"); return 1; }
            if (op_run(op, EPI_JACOBI3Z, omega, b, y, b, 0, 1, wn ? 1 : 0, stream, wd ? 1 : 0, 0, 0, route)) return 1;
            break;
        case EPI_APPLYDOT:
            if (x == y) { set_error("apply: y must not alias x"); return 1; }
            if (wn || !wd) { set_error("apply + dot: dot_out only"); return 1; }
            if (op_run(op, EPI_APPLYDOT, 0.0, x, y, x, zb, ze, 0, stream, 1, zb2, ze2, route)) return 1;
            break;
        default:
            set_error("poms_op_run_reduce: bad epilogue");
            return 1;
    }
    return 0;
}

namespace poms {
// The distributed operator call's two launches -- planes [ib, ie) on `stream`, then
// the boundary ranges [b1s, b1e) + [b2s, b2e) once the ghost exchange is done --
// with both launches' partials side by side in the scratch and ONE reduction per
// requested sum after both (one launch fewer per sum than reducing each launch;
// poms_op_run_dist).  The boundary launch goes to h.bstream when given (the
// communication stream, right behind the exchange): it depends on the exchange
// only, not on the interior launch, so its workgroups fill the CUs the interior
// launch's last round leaves idle instead of running as a separate, mostly empty
// round of its own; `stream` then waits for it (h.join) before the reductions.
int op_run_split(poms_op* op, int epilogue, double omega, const double* x, double* y, const double* b,
                 int64_t ib, int64_t ie, int64_t b1s, int64_t b1e, int64_t b2s, int64_t b2e, double* norm_out,
                 double* dot_out, const SplitHooks& h, void* stream) {
    if (!op) { set_error("op_run_split: null operator"); return 1; }
    if (general_form(op)) {   // its own partials layout: reduce each launch, both on `stream`
        if (poms_op_run_reduce2(op, epilogue, omega, x, y, b, ib, ie, 0, 0, norm_out, dot_out, 0, stream)) return 1;
        if (h.ghosts_on(h.arg, stream)) return 1;
        return poms_op_run_reduce2(op, epilogue, omega, x, y, b, b1s, b1e, b2s, b2e, norm_out, dot_out, 1, stream);
    }
    const bool wn = norm_out != nullptr, wd = dot_out != nullptr;
    struct Reset {
        poms_op* o;
        ~Reset() { o->part_off = 0; o->dot_base = -1; }
    } reset{op};
    op->part_off = 0;
    op->dot_base = kScratch / 2;
    op->split_interior = true;
    const int rci = op_run_epi(op, epilogue, omega, x, y, b, ib, ie, 0, 0, wn, wd, stream);
    op->split_interior = false;
    if (rci) return 1;
    const int64_t n1 = op->last_partials;
    void* bs = h.bstream ? h.bstream : stream;
    if (h.ghosts_on(h.arg, bs)) return 1;
    op->part_off = n1;
    if (op_run_epi(op, epilogue, omega, x, y, b, b1s, b1e, b2s, b2e, wn, wd, bs)) return 1;
    if (bs != stream && h.join(h.arg, bs, stream)) return 1;
    const int64_t n = n1 + op->last_partials;
    op->last_partials = 0;   // not in the layout poms_op_last_partials describes
    // (the reductions stay on `stream`: queued on the boundary stream behind the
    // boundary launch they added a second cross-queue wait per call -- loopback proxy
    // 41.7 -> 43.5 ms, profiles/r03/proxy/reductions_on_cs_REVERTED/)
    if ((wn && reduce_launch(op->ctx->scratch, (int)n, norm_out, as_stream(stream))) ||
        (wd && reduce_launch(op->ctx->scratch + kScratch / 2, (int)n, dot_out, as_stream(stream)))) {
        set_error("op_run_split: reduction launch failed");
        return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}
}  // namespace poms

extern "C" {

int poms_op_run_reduce2(poms_op* op, int epilogue, double omega, const double* x, double* y,
                        const double* b, int64_t zb, int64_t ze, int64_t zb2, int64_t ze2,
                        double* norm_out, double* dot_out, int accumulate, void* stream) {
    if (!op) { set_error("poms_op_run_reduce: null operator"); return 1; }
    const bool wn = norm_out != nullptr, wd = dot_out != nullptr;
    if (op_run_epi(op, epilogue, omega, x, y, b, zb, ze, zb2, ze2, wn, wd, stream)) return 1;
    const int64_t n = op->last_partials;
    if ((wn && reduce_launch(op->ctx->scratch, (int)n, norm_out, as_stream(stream), accumulate)) ||
        (wd && reduce_launch(op->ctx->scratch + n, (int)n, dot_out, as_stream(stream), accumulate))) {
        set_error("poms_op_run_reduce: reduction launch failed");
        return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_op_run_reduce(poms_op* op, int epilogue, double omega, const double* x, double* y,
                       const double* b, int64_t zb, int64_t ze, double* norm_out, double* dot_out,
                       int accumulate, void* stream) {
    return poms_op_run_reduce2(op, epilogue, omega, x, y, b, zb, ze, 0, 0, norm_out, dot_out, accumulate, stream);
}

int poms_op_last_partials(poms_op* op, int64_t* count) {
    if (!op || !count) { set_error("null argument"); return 1; }
    *count = op->last_partials;
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

int poms_op_timing(poms_op* op, int enable, int epilogue, int every, int reserve) {
    if (!op || every < 1 || reserve < 0) { set_error("poms_op_timing: bad argument"); return 1; }
    op->timing = enable != 0;
    if (!op->timing) return 0;   // disabling keeps the record for poms_op_timing_read
    op->tl_used = 0;
    op->t_epi = epilogue;
    op->t_every = every;
    op->t_seen = 0;
    POMS_HIP_CHECK(hipSetDevice(op->ctx->device));
    while (op->tl.size() < (size_t)reserve) {   // create the events now, not inside the timed work
        poms_op::TimedLaunch t{};
        POMS_HIP_CHECK(hipEventCreate(&t.e0));
        POMS_HIP_CHECK(hipEventCreate(&t.e1));
        op->tl.push_back(t);
    }
    return 0;
}

int poms_op_timing_read(poms_op* op, int epilogue, double* total_ms, int64_t* launches, int64_t* dofs) {
    if (!op || !total_ms || !launches || !dofs) { set_error("poms_op_timing_read: null argument"); return 1; }
    double tot = 0.0;
    int64_t n = 0, d = 0;
    for (size_t i = 0; i < op->tl_used; ++i) {
        const auto& t = op->tl[i];
        if (t.epi != epilogue) continue;
        POMS_HIP_CHECK(hipEventSynchronize(t.e1));
        float ms = 0.0f;
        POMS_HIP_CHECK(hipEventElapsedTime(&ms, t.e0, t.e1));
        tot += ms;
        ++n;
        d += t.ndof;
    }
    *total_ms = tot;
    *launches = n;
    *dofs = d;
    return 0;
}
