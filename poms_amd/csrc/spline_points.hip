// Spline fields at scattered points (gfx950): the positions are a DEVICE array that may
// change every step, so the span search (splines.find_span) and the Cox-de Boor triangle
// (splines.basis_funs_ders) run in the kernels, on the knots a handle uploaded once.
//
//   gather : u_h(x_k) = sum_a B0[a0] B1[a1] B2[a2] x[first + a], and its gradient
//   scatter: b[i] (+)= sum_k w_k B_i(x_k), the load vector of point sources
//
// Gather and the atomic scatter take one thread per point: the 1D rows live in registers
// (every loop is unrolled to the largest degree of the space and guarded by the axis'
// own), the Pi(p_d + 1) coefficients are p+1 consecutive doubles per (a0, a1).
//
// The binned scatter has no atomics.  The points arrive ordered by cell (perm,
// cell_start).  Stage 1 gives one wave to a cell: lane a owns local basis function
// a = (a0, a1, a2), the wave walks the cell's points in perm order 64 at a time -- each
// lane computes the 1D rows of ONE point of the batch into LDS, then every lane adds the
// batch's w B0[a0] B1[a1] B2[a2] to its running sum in that order -- and the cell's sums
// go to the handle's scratch.  Stage 2 gives one thread to a DOF: it adds the blocks of
// the cells in its support in lexicographic cell order and writes b[i].  The bits depend
// on the slabs of cells the caller walks (they cut the first used axis) and on the order
// of the points inside each cell, and on nothing else.
//
// Safety: an element index is clamped into [0, nel - 1] before anything is indexed with
// it, and the inside / outside verdict only selects between the result and zero (or
// drops the deposit), so no verdict can address outside the vector.
//
// Floating-point contraction is off in this file and every fused multiply-add is
// written out: the value / derivative chains of poms_points_eval are the same
// instructions whichever `what` is asked for, which makes the one-pass gradient equal
// the separate calls bitwise.
#include <algorithm>
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "launchers.hpp"     // (these two through abi_internal.hpp; named for the
#include "split_hooks.hpp"   // build's dependency scan, which reads this file only)
#include "abi_internal.hpp"
#include "poms_hip.h"

#pragma clang fp contract(off)

namespace poms {
namespace {

struct PtAxis {
    const double* T;     // knots (n + p + 1)
    const double* brk;   // breakpoints of the non-empty spans (nel + 1)
    const int* espan;    // span index of element e (nel)
    const int* elo;      // DOF i: elements [elo[i], ehi[i]) have i in their support (n)
    const int* ehi;
    double lo, hi;       // T[p], T[n]
    double inv_h;        // uniform: nel / (hi - lo)
    int p, n, nel, uniform;
};

struct PtGeom {
    PtAxis ax[3];
    int64_t base, s0, s1;   // offset of interior (0, 0, 0); plane and row strides
    int lead;               // unused leading axes (3 - ndim): no positions, one span, p = 0
    int nfun;               // Pi (p_d + 1)
};

// Element of x on one axis, always inside [0, nel - 1]; clears `inside` for x outside
// [lo, hi] and for NaN (every comparison with NaN is false).
__device__ __forceinline__ int locate(const PtAxis& A, double x, bool& inside) {
    inside = inside && (x >= A.lo) && (x <= A.hi);
    const int last = A.nel - 1;
    int e;
    if (A.uniform) {
        double g = (x - A.lo) * A.inv_h;
        g = fmin(fmax(g, 0.0), (double)last);   // fmax(NaN, 0) = 0
        e = (int)g;
        // the guess is a rounded product: the stored breakpoints decide
        while (e > 0 && x < A.brk[e]) --e;
        while (e < last && x >= A.brk[e + 1]) ++e;
    } else {
        int lo = 0, hi = A.nel;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (x < A.brk[mid]) hi = mid; else lo = mid;
        }
        e = lo;
    }
    return min(max(e, 0), last);
}

// The p+1 B-splines that are non-zero on `span` at x and their first derivatives: the
// triangle of basis_funs_ders.  The last level's quotients N_{r,p-1} / (T[span+r+1] -
// T[span+r+1-p]) are kept, D[r] = p (q[r-1] - q[r]).  Entries past p are 0.
template <int PM>
__device__ __forceinline__ void basis_1d(const double* __restrict__ T, int p, int span, double x,
                                         double (&N)[PM + 1], double (&D)[PM + 1]) {
    double left[PM + 1], right[PM + 1], q[PM + 1];
#pragma unroll
    for (int r = 0; r <= PM; ++r) { N[r] = 0.0; q[r] = 0.0; left[r] = 0.0; right[r] = 0.0; }
    N[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= PM; ++j) {
        if (j <= p) {
            left[j] = x - T[span + 1 - j];
            right[j] = T[span + j] - x;
            double saved = 0.0;
#pragma unroll
            for (int r = 0; r < j; ++r) {
                const double den = right[r + 1] + left[j - r];
                const double tmp = N[r] / den;
                if (j == p) q[r] = tmp;
                N[r] = saved + right[r + 1] * tmp;
                saved = left[j - r] * tmp;
            }
            N[j] = saved;
        }
    }
    const double fp = (double)p;
#pragma unroll
    for (int r = 0; r <= PM; ++r) {
        const double a = r >= 1 ? q[r - 1] : 0.0;   // q[p] stays 0
        D[r] = r <= p ? fp * (a - q[r]) : 0.0;
    }
}

// Rows of every axis at point k.  Unused leading axes: one function, value 1.
template <int PM>
__device__ __forceinline__ bool point_rows(const PtGeom& g, const double* __restrict__ pos, int64_t N, int64_t k,
                                           int (&e)[3], int (&first)[3], double (&Nv)[3][PM + 1],
                                           double (&Dv)[3][PM + 1]) {
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        e[d] = 0; first[d] = 0;
#pragma unroll
        for (int a = 0; a <= PM; ++a) { Nv[d][a] = a == 0 ? 1.0 : 0.0; Dv[d][a] = 0.0; }
        if (d >= g.lead) {
            const double xd = pos[(int64_t)(d - g.lead) * N + k];
            e[d] = locate(g.ax[d], xd, inside);
            const int span = g.ax[d].espan[e[d]];
            basis_1d<PM>(g.ax[d].T, g.ax[d].p, span, xd, Nv[d], Dv[d]);
            first[d] = span - g.ax[d].p;
        }
    }
    return inside;
}

__global__ void __launch_bounds__(256)
points_cells_kernel(PtGeom g, const double* __restrict__ pos, int64_t N, int64_t* __restrict__ cell) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    bool inside = true;
    int64_t c = 0;
    for (int d = g.lead; d < 3; ++d)
        c = c * g.ax[d].nel + locate(g.ax[d], pos[(int64_t)(d - g.lead) * N + k], inside);
    cell[k] = inside ? c : -1;
}

// sum_a A[a] v[a] over a <= p: a product, then fused multiply-adds in ascending a
#define POMS_PT_CHAIN(acc, A, v, a, p) acc = (a) == 0 ? (A) * (v) : ((a) <= (p) ? fma((A), (v), acc) : acc)

// One thread per point.  GRAD: value and every first derivative from one load of the
// coefficients, out[(1 + ndim), N]; else the value (der < 0) or the derivative along
// axis `der` (0..2, an index of the three stored axes), out[N].
template <int PM, bool GRAD>
__global__ void __launch_bounds__(256)
points_eval_kernel(PtGeom g, const double* __restrict__ x, const double* __restrict__ pos, int64_t N, int der,
                   double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    int e[3], first[3];
    double Nv[3][PM + 1], Dv[3][PM + 1];
    const bool inside = point_rows<PM>(g, pos, N, k, e, first, Nv, Dv);
    const int nd = 3 - g.lead;
    if (!inside) {
        out[k] = 0.0;
        if (GRAD)
            for (int d = 0; d < nd; ++d) out[(int64_t)(1 + d) * N + k] = 0.0;
        return;
    }
    const int p0 = g.ax[0].p, p1 = g.ax[1].p, p2 = g.ax[2].p;
    const double* xp = x + g.base + first[0] * g.s0 + first[1] * g.s1 + first[2];
    if (GRAD) {
        double v = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
        for (int a0 = 0; a0 <= PM; ++a0) {
            if (a0 > p0) continue;
            double u = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
            for (int a1 = 0; a1 <= PM; ++a1) {
                if (a1 > p1) continue;
                const double* row = xp + a0 * g.s0 + a1 * g.s1;
                double r = 0.0, rd = 0.0;
#pragma unroll
                for (int a2 = 0; a2 <= PM; ++a2) {
                    if (a2 > p2) continue;
                    const double c = row[a2];
                    POMS_PT_CHAIN(r, Nv[2][a2], c, a2, p2);
                    POMS_PT_CHAIN(rd, Dv[2][a2], c, a2, p2);
                }
                POMS_PT_CHAIN(u, Nv[1][a1], r, a1, p1);
                POMS_PT_CHAIN(u1, Dv[1][a1], r, a1, p1);
                POMS_PT_CHAIN(u2, Nv[1][a1], rd, a1, p1);
            }
            POMS_PT_CHAIN(v, Nv[0][a0], u, a0, p0);
            POMS_PT_CHAIN(g0, Dv[0][a0], u, a0, p0);
            POMS_PT_CHAIN(g1, Nv[0][a0], u1, a0, p0);
            POMS_PT_CHAIN(g2, Nv[0][a0], u2, a0, p0);
        }
        out[k] = v;
        const double gr[3] = {g0, g1, g2};
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d >= g.lead) out[(int64_t)(1 + d - g.lead) * N + k] = gr[d];
    } else {
        double A[3][PM + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int a = 0; a <= PM; ++a) A[d][a] = der == d ? Dv[d][a] : Nv[d][a];
        double v = 0.0;
#pragma unroll
        for (int a0 = 0; a0 <= PM; ++a0) {
            if (a0 > p0) continue;
            double u = 0.0;
#pragma unroll
            for (int a1 = 0; a1 <= PM; ++a1) {
                if (a1 > p1) continue;
                const double* row = xp + a0 * g.s0 + a1 * g.s1;
                double r = 0.0;
#pragma unroll
                for (int a2 = 0; a2 <= PM; ++a2) {
                    if (a2 > p2) continue;
                    POMS_PT_CHAIN(r, A[2][a2], row[a2], a2, p2);
                }
                POMS_PT_CHAIN(u, A[1][a1], r, a1, p1);
            }
            POMS_PT_CHAIN(v, A[0][a0], u, a0, p0);
        }
        out[k] = v;
    }
}

// b[first + a] += w B0[a0] B1[a1] B2[a2]: one thread per point, one FP64 atomic add per
// local basis function.
template <int PM>
__global__ void __launch_bounds__(256)
points_deposit_atomic_kernel(PtGeom g, const double* __restrict__ pos, const double* __restrict__ w, int64_t N,
                             double* __restrict__ b) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    int e[3], first[3];
    double Nv[3][PM + 1], Dv[3][PM + 1];
    if (!point_rows<PM>(g, pos, N, k, e, first, Nv, Dv)) return;
    const double wk = w ? w[k] : 1.0;
    const int p0 = g.ax[0].p, p1 = g.ax[1].p, p2 = g.ax[2].p;
    double* bp = b + g.base + first[0] * g.s0 + first[1] * g.s1 + first[2];
#pragma unroll
    for (int a0 = 0; a0 <= PM; ++a0) {
        if (a0 > p0) continue;
        const double w0 = wk * Nv[0][a0];
#pragma unroll
        for (int a1 = 0; a1 <= PM; ++a1) {
            if (a1 > p1) continue;
            const double w01 = w0 * Nv[1][a1];
            double* row = bp + a0 * g.s0 + a1 * g.s1;
#pragma unroll
            for (int a2 = 0; a2 <= PM; ++a2) {
                if (a2 > p2) continue;
                unsafeAtomicAdd(row + a2, w01 * Nv[2][a2]);
            }
        }
    }
}

// Binned scatter, stage 1: workgroup = one wave = one cell of the slab that starts at cell
// c0.  rows[pt] holds the three 1D value rows of the batch's point pt and its weight.
template <int PM>
__global__ void __launch_bounds__(64)
points_bin_cells_kernel(PtGeom g, const double* __restrict__ pos, const double* __restrict__ w, int64_t N,
                        const int64_t* __restrict__ perm, const int64_t* __restrict__ cell_start, int64_t c0,
                        double* __restrict__ scratch) {
    constexpr int R = PM + 1;
    constexpr int NJ = (R * R * R + 63) / 64;   // basis functions per lane
    constexpr int W = 3 * R + 1;                // odd: lanes write their rows to different banks
    __shared__ double rows[64][W];
    const int lane = threadIdx.x;
    const int64_t cl = blockIdx.x, c = c0 + cl;
    const int nel1 = g.ax[1].nel, nel2 = g.ax[2].nel;
    const int ce[3] = {(int)(c / ((int64_t)nel1 * nel2)), (int)((c / nel2) % nel1), (int)(c % nel2)};
    int span[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) span[d] = g.ax[d].espan[min(max(ce[d], 0), g.ax[d].nel - 1)];
    const int r1 = g.ax[1].p + 1, r2 = g.ax[2].p + 1;
    int i0[NJ], i1[NJ], i2[NJ];
    double acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int kk = min(lane + 64 * j, g.nfun - 1);
        i0[j] = kk / (r1 * r2);
        i1[j] = R + (kk / r2) % r1;
        i2[j] = 2 * R + kk % r2;
        acc[j] = 0.0;
    }
    const int64_t cs = min(max(cell_start[c], (int64_t)0), N);
    const int64_t cend = min(max(cell_start[c + 1], cs), N);
    for (int64_t b0 = cs; b0 < cend; b0 += 64) {
        const int cnt = (int)min((int64_t)64, cend - b0);
        if (lane < cnt) {
            const int64_t k = perm[b0 + lane];
            const bool ok = k >= 0 && k < N;   // a bad permutation deposits nothing
            rows[lane][3 * R] = ok ? (w ? w[k] : 1.0) : 0.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                double Nd[R], Dd[R];
#pragma unroll
                for (int a = 0; a < R; ++a) Nd[a] = a == 0 ? 1.0 : 0.0;
                if (d >= g.lead) {
                    const double xd = ok ? pos[(int64_t)(d - g.lead) * N + k] : g.ax[d].lo;
                    basis_1d<PM>(g.ax[d].T, g.ax[d].p, span[d], xd, Nd, Dd);
                }
#pragma unroll
                for (int a = 0; a < R; ++a) rows[lane][d * R + a] = Nd[a];
            }
        }
        __syncthreads();
        for (int pt = 0; pt < cnt; ++pt) {
            const double* rp = rows[pt];
            const double wk = rp[3 * R];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = fma((wk * rp[i0[j]]) * rp[i1[j]], rp[i2[j]], acc[j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int kk = lane + 64 * j;
        if (kk < g.nfun) scratch[cl * g.nfun + kk] = acc[j];
    }
}

// Binned scatter, stage 2: one thread per DOF adds the blocks of the cells in its support
// whose element along the first used axis lies in [eb, ee) (the slab, cells from c0 on),
// in lexicographic cell order.
__global__ void __launch_bounds__(256)
points_bin_dofs_kernel(PtGeom g, const double* __restrict__ scratch, int64_t c0, int eb, int ee, int accumulate,
                       double* __restrict__ b) {
    const int n0 = g.ax[0].n, n1 = g.ax[1].n, n2 = g.ax[2].n;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n0 * n1 * n2) return;
    const int j2 = (int)(t % n2), j1 = (int)((t / n2) % n1), j0 = (int)(t / ((int64_t)n1 * n2));
    int lo0 = g.ax[0].elo[j0], hi0 = g.ax[0].ehi[j0];
    int lo1 = g.ax[1].elo[j1], hi1 = g.ax[1].ehi[j1];
    int lo2 = g.ax[2].elo[j2], hi2 = g.ax[2].ehi[j2];
    if (g.lead == 0) { lo0 = max(lo0, eb); hi0 = min(hi0, ee); }
    else if (g.lead == 1) { lo1 = max(lo1, eb); hi1 = min(hi1, ee); }
    else { lo2 = max(lo2, eb); hi2 = min(hi2, ee); }
    if (accumulate && (lo0 >= hi0 || lo1 >= hi1 || lo2 >= hi2)) return;
    const int r1 = g.ax[1].p + 1, r2 = g.ax[2].p + 1;
    const int nel1 = g.ax[1].nel, nel2 = g.ax[2].nel;
    double s = 0.0;
    for (int e0 = lo0; e0 < hi0; ++e0) {
        const int a0 = j0 - (g.ax[0].espan[e0] - g.ax[0].p);
        for (int e1 = lo1; e1 < hi1; ++e1) {
            const int a1 = j1 - (g.ax[1].espan[e1] - g.ax[1].p);
            for (int e2 = lo2; e2 < hi2; ++e2) {
                const int a2 = j2 - (g.ax[2].espan[e2] - g.ax[2].p);
                const int64_t cl = ((int64_t)e0 * nel1 + e1) * nel2 + e2 - c0;
                s += scratch[cl * g.nfun + (a0 * r1 + a1) * r2 + a2];
            }
        }
    }
    double* o = b + g.base + j0 * g.s0 + j1 * g.s1 + j2;
    *o = accumulate ? *o + s : s;
}

template <typename T>
int upload_tab(const std::vector<T>& h, T** dev) {
    POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(dev), std::max<size_t>(h.size(), 1) * sizeof(T)));
    if (!h.empty()) POMS_HIP_CHECK(hipMemcpy(*dev, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace
}  // namespace poms

using namespace poms;

struct poms_points {
    poms_ctx* ctx = nullptr;
    int ndim = 3, pmax = 1;
    PtGeom g{};
    int64_t ncells = 1;
    int64_t max_slab = 1;     // elements of the first used axis whose cells fit the scratch
    int64_t slab_cells = 1;   // cells per such element
    double* T[3]{};
    double* brk[3]{};
    int *espan[3]{}, *elo[3]{}, *ehi[3]{};
    double* scratch = nullptr;
};

namespace {

constexpr int64_t kMaxPoints = (int64_t)1 << 38;   // 256 points per block, 2^30 blocks

bool run_ok(const char* what, const poms_points* h, const void* pos, int64_t N) {
    const std::string w(what);
    if (!h) { set_error(w + ": null handle"); return false; }
    if (N < 0 || N > kMaxPoints) { set_error(w + ": N outside [0, 2^38]"); return false; }
    if (N > 0 && !pos) { set_error(w + ": null positions"); return false; }
    return true;
}

unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

template <int PM>
void eval_pm(const poms_points* h, const double* x, const double* pos, int64_t N, int what, double* out,
             hipStream_t st) {
    const dim3 grid(blocks256(N)), block(256);
    if (what < 0)
        hipLaunchKernelGGL((points_eval_kernel<PM, true>), grid, block, 0, st, h->g, x, pos, N, -1, out);
    else
        hipLaunchKernelGGL((points_eval_kernel<PM, false>), grid, block, 0, st, h->g, x, pos, N,
                           what == 0 ? -1 : h->g.lead + what - 1, out);
}

template <int PM>
void bin_cells_pm(const poms_points* h, const double* pos, const double* w, int64_t N, const int64_t* perm,
                  const int64_t* cell_start, int64_t c0, int64_t nc, hipStream_t st) {
    hipLaunchKernelGGL(points_bin_cells_kernel<PM>, dim3((unsigned)nc), dim3(64), 0, st, h->g, pos, w, N, perm,
                       cell_start, c0, h->scratch);
}

}  // namespace

#define POMS_PT_SWITCH(pm, CALL)                                  \
    switch (pm) {                                                 \
        case 1: CALL(1); break;                                   \
        case 2: CALL(2); break;                                   \
        case 3: CALL(3); break;                                   \
        case 4: CALL(4); break;                                   \
        default: CALL(5); break;                                  \
    }

extern "C" {

int poms_points_destroy(poms_points* h) {
    if (!h) return 0;
    for (int d = 0; d < 3; ++d) {
        if (h->T[d]) (void)hipFree(h->T[d]);
        if (h->brk[d]) (void)hipFree(h->brk[d]);
        if (h->espan[d]) (void)hipFree(h->espan[d]);
        if (h->elo[d]) (void)hipFree(h->elo[d]);
        if (h->ehi[d]) (void)hipFree(h->ehi[d]);
    }
    if (h->scratch) (void)hipFree(h->scratch);
    delete h;
    return 0;
}

int poms_points_create(poms_ctx* ctx, int ndim, const poms_layout* layout, const int* p, const int64_t* nknots,
                       const double* const* knots, int64_t scratch_bytes, poms_points** out) {
    if (!ctx || !layout || !p || !nknots || !knots || !out) { set_error("poms_points_create: null argument"); return 1; }
    if (ndim < 1 || ndim > 3) { set_error("poms_points_create: ndim 1..3"); return 1; }
    if (!layout_ok(layout)) { set_error("poms_points_create: bad layout"); return 1; }
    if (scratch_bytes < 8) { set_error("poms_points_create: scratch_bytes >= 8"); return 1; }
    const int lead = 3 - ndim;
    std::vector<double> brk[3];
    std::vector<int> espan[3], elo[3], ehi[3];
    bool uniform[3]{};
    for (int d = 0; d < 3; ++d) {
        const int P = p[d];
        const int64_t nk = nknots[d];
        const double* T = knots[d];
        if (!T || P < (d < lead ? 0 : 1) || P > 5 || nk < 2 * (P + 1) || nk > 0x3fffffff) {
            set_error("poms_points_create: bad axis (knots, degree 1..5, at least 2 (p + 1) knots)");
            return 1;
        }
        const int64_t n = nk - P - 1;
        if (n != layout->n[d] || P != layout->pads[d]) {
            set_error("poms_points_create: nknots - p - 1 must be layout->n and p must be layout->pads");
            return 1;
        }
        if (d < lead && (n != 1 || P != 0)) {
            set_error("poms_points_create: unused leading axes need two knots, p = 0, n = 1, pad = 0");
            return 1;
        }
        for (int64_t i = 0; i < nk; ++i)
            if (!std::isfinite(T[i]) || (i && T[i] < T[i - 1])) {
                set_error("poms_points_create: knots must be finite and non-decreasing");
                return 1;
            }
        if (T[0] != T[P] || T[n] != T[nk - 1] || !(T[P] < T[n])) {
            set_error("poms_points_create: knots must be open (p + 1 equal knots at both ends)");
            return 1;
        }
        // the non-empty spans of [p, n): breakpoints and the span of each element
        for (int64_t s = P; s < n; ++s)
            if (T[s + 1] > T[s]) { espan[d].push_back((int)s); brk[d].push_back(T[s]); }
        brk[d].push_back(T[n]);
        const int nel = (int)espan[d].size();
        const double h0 = (T[n] - T[P]) / nel;
        uniform[d] = true;
        for (int e = 0; e < nel; ++e)
            if (std::fabs((brk[d][e + 1] - brk[d][e]) - h0) > 1e-9 * h0) uniform[d] = false;
        // elements whose span s has s - p <= i <= s
        elo[d].resize((size_t)n); ehi[d].resize((size_t)n);
        int a = 0, b = 0;
        for (int64_t i = 0; i < n; ++i) {
            while (a < nel && espan[d][a] < i) ++a;
            while (b < nel && espan[d][b] <= i + P) ++b;
            elo[d][(size_t)i] = a; ehi[d][(size_t)i] = b;
        }
    }
    POMS_HIP_CHECK(hipSetDevice(ctx_device(ctx)));
    poms_points* h = new poms_points;
    h->ctx = ctx;
    h->ndim = ndim;
    PtGeom& g = h->g;
    g.lead = lead;
    g.s1 = layout->pitch > 0 ? layout->pitch : layout->n[2] + 2 * layout->pads[2];
    g.s0 = (layout->n[1] + 2 * layout->pads[1]) * g.s1;
    g.base = layout->pads[0] * g.s0 + layout->pads[1] * g.s1 + layout->pads[2];
    g.nfun = 1;
    int rc = 0;
    for (int d = 0; d < 3 && !rc; ++d) {
        const int P = p[d];
        const int64_t nk = nknots[d], n = nk - P - 1;
        PtAxis& A = g.ax[d];
        A.p = P; A.n = (int)n; A.nel = (int)espan[d].size(); A.uniform = uniform[d] ? 1 : 0;
        A.lo = knots[d][P]; A.hi = knots[d][n];
        A.inv_h = A.nel / (A.hi - A.lo);
        g.nfun *= P + 1;
        h->pmax = std::max(h->pmax, P);
        h->ncells *= A.nel;
        rc = upload_tab(std::vector<double>(knots[d], knots[d] + nk), &h->T[d]) || upload_tab(brk[d], &h->brk[d]) ||
             upload_tab(espan[d], &h->espan[d]) || upload_tab(elo[d], &h->elo[d]) || upload_tab(ehi[d], &h->ehi[d]);
        A.T = h->T[d]; A.brk = h->brk[d]; A.espan = h->espan[d]; A.elo = h->elo[d]; A.ehi = h->ehi[d];
    }
    if (!rc) {
        // slabs cut the first used axis: contiguous ranges of the C-order cell index
        h->slab_cells = h->ncells / g.ax[lead].nel;
        const int64_t per_e0 = h->slab_cells * g.nfun * (int64_t)sizeof(double);
        h->max_slab = std::min<int64_t>(g.ax[lead].nel, scratch_bytes / per_e0);
        if (h->max_slab < 1) {
            set_error("poms_points_create: scratch_bytes below one slab of cells (one element of the first axis: "
                      "the other axes' cells times Pi(p+1) doubles)");
            rc = 1;
        } else if (h->max_slab * h->slab_cells > 0x7fffffff) {
            set_error("poms_points_create: more than 2^31 cells in one slab");
            rc = 1;
        } else if (hipMalloc(reinterpret_cast<void**>(&h->scratch), (size_t)(h->max_slab * per_e0)) != hipSuccess) {
            set_error("poms_points_create: allocation of the scratch failed");
            rc = 1;
        }
    }
    if (rc) { poms_points_destroy(h); return 1; }
    *out = h;
    return 0;
}

int poms_points_info(poms_points* h, int64_t* info) {
    if (!h) { set_error("poms_points_info: null handle"); return 1; }
    if (!info) { set_error("poms_points_info: null argument"); return 1; }
    info[0] = h->ncells;
    info[1] = h->max_slab;
    for (int d = 0; d < 3; ++d) { info[2 + d] = h->g.ax[d].nel; info[5 + d] = h->g.ax[d].uniform; }
    return 0;
}

int poms_points_cells(poms_points* h, const double* pos, int64_t N, int64_t* cell, void* stream) {
    if (!run_ok("poms_points_cells", h, pos, N)) return 1;
    if (N == 0) return 0;
    if (!cell) { set_error("poms_points_cells: null argument"); return 1; }
    hipLaunchKernelGGL(points_cells_kernel, dim3(blocks256(N)), dim3(256), 0, as_stream(stream), h->g, pos, N, cell);
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_points_eval(poms_points* h, const double* x, const double* pos, int64_t N, int what, double* out,
                     void* stream) {
    if (!run_ok("poms_points_eval", h, pos, N)) return 1;
    if (what < -1 || what > h->ndim) { set_error("poms_points_eval: what must be -1, 0 or 1 + axis"); return 1; }
    if (N == 0) return 0;
    if (!x || !out) { set_error("poms_points_eval: null argument"); return 1; }
    hipStream_t st = as_stream(stream);
#define POMS_PT_EVAL(PM) eval_pm<PM>(h, x, pos, N, what, out, st)
    POMS_PT_SWITCH(h->pmax, POMS_PT_EVAL)
#undef POMS_PT_EVAL
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_points_deposit_atomic(poms_points* h, const double* pos, const double* w, int64_t N, double* b,
                               void* stream) {
    if (!run_ok("poms_points_deposit_atomic", h, pos, N)) return 1;
    if (N == 0) return 0;
    if (!b) { set_error("poms_points_deposit_atomic: null argument"); return 1; }
    hipStream_t st = as_stream(stream);
#define POMS_PT_ATOMIC(PM) \
    hipLaunchKernelGGL(points_deposit_atomic_kernel<PM>, dim3(blocks256(N)), dim3(256), 0, st, h->g, pos, w, N, b)
    POMS_PT_SWITCH(h->pmax, POMS_PT_ATOMIC)
#undef POMS_PT_ATOMIC
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_points_deposit_binned(poms_points* h, const double* pos, const double* w, int64_t N, const int64_t* perm,
                               const int64_t* cell_start, int64_t e0b, int64_t e0e, int accumulate, double* b,
                               void* stream) {
    if (!run_ok("poms_points_deposit_binned", h, pos, N)) return 1;
    if (e0b < 0 || e0e < e0b || e0e > h->g.ax[h->g.lead].nel) {
        set_error("poms_points_deposit_binned: slab outside [0, nel] of the first axis");
        return 1;
    }
    if (e0e - e0b > h->max_slab) { set_error("poms_points_deposit_binned: slab exceeds the handle's scratch"); return 1; }
    if (!b || !cell_start || (N > 0 && !perm)) { set_error("poms_points_deposit_binned: null argument"); return 1; }
    if (e0e == e0b && accumulate) return 0;
    hipStream_t st = as_stream(stream);
    const int64_t c0 = e0b * h->slab_cells, nc = (e0e - e0b) * h->slab_cells;
    if (nc > 0) {
#define POMS_PT_BIN(PM) bin_cells_pm<PM>(h, pos, w, N, perm, cell_start, c0, nc, st)
        POMS_PT_SWITCH(h->pmax, POMS_PT_BIN)
#undef POMS_PT_BIN
    }
    const int64_t ndof = (int64_t)h->g.ax[0].n * h->g.ax[1].n * h->g.ax[2].n;
    if (ndof > kMaxPoints) { set_error("poms_points_deposit_binned: vector too large for one launch"); return 1; }
    hipLaunchKernelGGL(points_bin_dofs_kernel, dim3(blocks256(ndof)), dim3(256), 0, st, h->g, h->scratch, c0,
                       (int)e0b, (int)e0e, accumulate ? 1 : 0, b);
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
