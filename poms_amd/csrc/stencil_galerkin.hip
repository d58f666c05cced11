// Galerkin coarsening of a general stencil operator: the reference forms
// `Ac = R.dot(Af).dot(P)` from the assembled matrix (`sources/mg_jac.py:80-81`).
// With P = P0 (x) P1 (x) P2 (knot insertion per axis) and A a stencil of half-widths
// p_d, Ac = P^T A P is again a stencil of half-widths p_d on the coarse space and
// is formed one axis at a time,
//     S'[.., I, .., kc, ..] = sum_{i, k} P_d[i, I] P_d[i + k - p, I + kc - p] S[.., i, .., k, ..],
// the weights being separable although A is not.
//
// One gather pass per axis over the coefficient planes [k0][k1][k2][i0][i1][i2]
// (plane k of row lin at coef[k * cstride + lin], as stencil_kernel reads them):
// one thread per (output row, offsets on the other two axes) keeps the 2p+1 output
// offsets of the pass's axis in registers, so the cnt (2p+1) loads of its support
// feed 2p+1 outputs.  Rows are fastest across lanes: the axis-0 and axis-1 passes
// read whole contiguous rows of each plane, the axis-2 pass (stride ~2 between lanes)
// runs last, on the array the other two already reduced.  The weights come from a
// host-built table wt[I][ii][k][kc] = P[lo[I] + ii, I] * P[lo[I] + ii + k - p, I + kc - p]
// (0 where the column or the row is outside the grid), which is what lets the
// kernel index unguarded: abi_op_setup.hip validates the factors before any launch.  In the
// axis-0 and axis-1 passes nearly every lane of a wave has the same I and reads the same
// weight; in the axis-2 pass the lanes differ in I, and its table is stored with the
// columns contiguous (wt[e][I], GalerkinPass::ws_col = 1) so that consecutive lanes read
// consecutive doubles (3.06 -> 2.13 ms at 3D p = 3 128^3 cells).
// No atomics: every output entry is one fixed fma chain (bitwise reproducible).
#include "common.hpp"
#include "launchers.hpp"

namespace poms {

// COLS: the table with the columns contiguous (entry stride ws_ent); otherwise a column's
// entries are contiguous and the compiler merges their loads
template <int W, bool COLS>
__global__ void __launch_bounds__(256)
galerkin_pass_kernel(const GalerkinPass g, const double* __restrict__ in, double* __restrict__ out) {
    constexpr int P = W / 2;
    const int d = g.d;
    const int wo = (g.w[0] * g.w[1] * g.w[2]) / W;   // offsets on the other two axes
    const int64_t total = g.cst_out * wo;
    const int nin_d = g.nin[d], nout_d = g.nout[d];
    // strides of the pass's axis: rows (input) and offset planes
    const int64_t istr = d == 0 ? (int64_t)g.nin[1] * g.nin[2] : d == 1 ? g.nin[2] : 1;
    const int kstr = d == 0 ? g.w[1] * g.w[2] : d == 1 ? g.w[2] : 1;
    for (int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x; tid < total; tid += (int64_t)gridDim.x * 256) {
        const int64_t lin = tid % g.cst_out;
        const int ko = (int)(tid / g.cst_out);
        const int I2 = (int)(lin % g.nout[2]);
        const int64_t t = lin / g.nout[2];
        const int I1 = (int)(t % g.nout[1]), I0 = (int)(t / g.nout[1]);
        int I, kbase;
        int64_t rin;   // input row with the pass's axis at 0
        if (d == 0) {
            I = I0;
            kbase = ko;   // (k1, k2)
            rin = (int64_t)I1 * g.nin[2] + I2;
        } else if (d == 1) {
            I = I1;
            kbase = (ko / g.w[2]) * g.w[1] * g.w[2] + ko % g.w[2];   // (k0, k2)
            rin = (int64_t)I0 * g.nin[1] * g.nin[2] + I2;
        } else {
            I = I2;
            kbase = ko * g.w[2];   // (k0, k1)
            rin = ((int64_t)I0 * g.nin[1] + I1) * g.nin[2];
        }
        const int l = g.lo[I], c = g.cnt[I];
        const double* __restrict__ wp = g.wt + (int64_t)I * g.ws_col;
        double acc[W];
#pragma unroll
        for (int kc = 0; kc < W; ++kc) acc[kc] = 0.0;
        for (int ii = 0; ii < c; ++ii) {
            const int i = l + ii;
            const double* src = in + (int64_t)kbase * g.cst_in + rin + i * istr;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int j = i + k - P;
                // (a fine coupling outside the grid is never read: its weight is 0 and
                // its storage need not be)
                const double s = (j >= 0 && j < nin_d) ? src[(int64_t)k * kstr * g.cst_in] : 0.0;
#pragma unroll
                for (int kc = 0; kc < W; ++kc)
                    acc[kc] = fma(wp[COLS ? (int64_t)((ii * W + k) * W + kc) * g.ws_ent : (ii * W + k) * W + kc], s, acc[kc]);
            }
        }
        double* dst = out + (int64_t)kbase * g.cst_out + lin;
#pragma unroll
        for (int kc = 0; kc < W; ++kc) {
            const int J = I + kc - P;
            dst[(int64_t)kc * kstr * g.cst_out] = (J >= 0 && J < nout_d) ? acc[kc] : 0.0;
        }
    }
}

template <int W>
static void galerkin_pass(bool cols, const GalerkinPass& g, const double* in, double* out, dim3 grid, hipStream_t st) {
    if (cols)
        hipLaunchKernelGGL((galerkin_pass_kernel<W, true>), grid, dim3(256), 0, st, g, in, out);
    else
        hipLaunchKernelGGL((galerkin_pass_kernel<W, false>), grid, dim3(256), 0, st, g, in, out);
}

int galerkin_pass_launch(const GalerkinPass& g, const double* in, double* out, hipStream_t st) {
    const int W = g.w[g.d];
    const int64_t total = g.cst_out * ((int64_t)(g.w[0] * g.w[1] * g.w[2]) / W);
    if (total == 0) return 0;
    const dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)1 << 20));
    const bool cols = g.ws_ent != 1;
    switch (W) {
        case 1: galerkin_pass<1>(cols, g, in, out, grid, st); break;
        case 3: galerkin_pass<3>(cols, g, in, out, grid, st); break;
        case 5: galerkin_pass<5>(cols, g, in, out, grid, st); break;
        case 7: galerkin_pass<7>(cols, g, in, out, grid, st); break;
        case 9: galerkin_pass<9>(cols, g, in, out, grid, st); break;
        case 11: galerkin_pass<11>(cols, g, in, out, grid, st); break;
        default:
            set_error("galerkin pass: stencil half-width above 5");
            return 1;
    }
    return 0;
}

}  // namespace poms
