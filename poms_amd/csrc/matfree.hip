// Matrix-free variable-coefficient operator: y = A x for -div(a grad u) + c u on a
// tensor B-spline space without a stored matrix,
//     (A x)_i = sum_q w_q [ c(q) u_h(q) phi_i(q) + a(q) grad u_h(q) . grad phi_i(q) ],
// the operator the reference assembles element by element
// (`sources/matrix_assembler.py:84-179`) and that its cycle needs only as `A.dot`, its
// diagonal and the residual (`sources/mg_jac.py:84-119`).  One launch per call:
// evaluation at the quadrature points, the pointwise scaling and the load-vector
// contraction are sum-factorised per axis and fused, so the point values live in LDS
// only.  HBM traffic per call: x (with the tile halo), a_q and c_q once each, the
// stored diagonal and b where the epilogue reads them, and y.
//
// A workgroup (256 threads) owns an 8 x 8 tile of output columns on axes 1 and 2 and a
// chunk [z0, z1) of output planes on axis 0, along which it marches one element at a
// time (2D: one trivial element, p = 0, one point of weight 1).  Per quadrature plane
// q0 of the element:
//   A  the rolling p0+1 planes of the x window (LDS ring) with B0[q0], B0'[q0]  -> sU
//   B  expand along axis 1: (B1 U, B1 U', B1' U)                                -> sT
//   C  one wave per q1 row, one lane per q2: u, d0u, d1u, d2u at the points, times
//      w c and w a                                               -> sG (the wave's row)
//   D  the same wave gathers the row along axis 2 into three arrays              -> sH
//   E  one thread per output column gathers along axis 1 into two values and
//   F  adds b0' V0 + b0 V1 to the p0+1 rolling output planes (sY, thread-private).
// The tile's slices of the axis-1 and axis-2 tables (basis values, weights, first
// functions) are staged in LDS once per tile, so the stages read no table from global
// memory; a_q and c_q of a wave's next row are fetched a round ahead.
// An output plane is final when the last element of its support has passed; the
// epilogue (the general stencil's: apply, residual, Jacobi, apply + dot, Chebyshev step)
// runs there.
// Every output is owned by one thread and summed in a fixed order, there are no
// atomics, and the per-block partial sums go through the usual reduction: two calls
// give the same bits.  Only interior entries of y are stored; x is read inside its
// window, which lies in the interior of its storage.
//
// TENSOR builds apply -div(G grad u) + c u with a full symmetric tensor G at the points
// (a mapped domain, G = a |det J| J^-1 J^-T, or anisotropic diffusion): a_q is then the
// array of component planes (common.hpp, Tensor6), and only stage C and its prefetch
// differ -- a wave fetches the tensor's entries and c_q of its next row a round ahead and
// writes the three fluxes f_i = w (g_i0 d0u + g_i1 d1u + g_i2 d2u) where w a d_iu goes
// otherwise.  A 2D operator's entries on axis 0 are not read and count as 0.
//
// The host (poms_op_create_matfree) checks every table entry the kernel indexes with
// and that every tile's window fits the LDS arrays below.
#include "common.hpp"
#include "launchers.hpp"

#include <algorithm>

namespace poms {

constexpr int MF_D = 8;                          // tile edge (output columns) on axes 1, 2
constexpr int MF_PMAX = 3, MF_NQMAX = 5;
constexpr int MF_W = MF_D + 2 * MF_PMAX;         // widest x window of a tile (14)
constexpr int MF_E = MF_D + MF_PMAX;             // most elements a tile touches per axis (11)
constexpr int MF_Q = MF_E * MF_NQMAX;            // most quadrature points per axis (55)
constexpr int MF_WW = MF_W * MF_W, MF_QW = MF_Q * MF_W, MF_DD = MF_D * MF_D;
static_assert(MF_W <= 16 && 3 * MF_D <= 64 && MF_Q <= 64, "the thread mappings of the stages");

int matfree_tile() { return MF_D; }
int matfree_max_window() { return MF_W; }
int matfree_max_elements() { return MF_E; }

// MASK builds apply Dirichlet faces (g.dmask, bit 2 axis + side): the constrained entries of
// x enter the window as 0 and a constrained output row takes diag * x.  The face set is a
// run-time field; MASK only says whether there is one, so that an operator without faces
// runs the code it ran before the mask existed.  (As a run-time test alone the mask cost the
// unmasked 2D apply 2 %: the kernel sits at the scalar-register limit, and the masked
// blocks moved another hundred scalar reads and writes into vector lanes, 229 / 116 against
// 136 / 69 in the scalar APPLY build.  The second set of builds adds 4 s to this file's
// compilation, which runs beside kron_v5.hip's 280 s.)
//
// FACE builds add the face terms of poms_op_add_face_term (F.mask, bit 2 axis + side; the face
// mass of a Robin condition) where an output plane is final: a row on such a face adds
// sum_k S[row, k] x[neighbour] over the face's (d-1)-dimensional stencil, x read from global
// memory.  As with MASK, FACE only says whether there is a face term, so that an operator
// without one runs the code it ran before.
template <int AX, bool MASK>
__device__ __forceinline__ double face_row(double s, const double* __restrict__ S, const MatfreeGeom& g, int pa, int pb,
                                           int i0, int i1, int i2, const double* __restrict__ x, int64_t xo) {
    constexpr int A = AX == 0 ? 1 : 0, B = AX == 2 ? 1 : 2;   // the face's two axes in increasing order
    const int n[3] = {g.n0, g.n1, g.n2}, i[3] = {i0, i1, i2};
    const int64_t st[3] = {g.s0, g.s1, 1};
    const int na = n[A], nb = n[B], ra = i[A], rb = i[B], wb = 2 * pb + 1;
    const double* Sr = S + ((int64_t)ra * nb + rb) * (2 * pa + 1) * wb;
    for (int ka = 0; ka <= 2 * pa; ++ka) {
        const int ja = ra + ka - pa;
        // neighbours outside the grid are skipped, and so are those on a constrained face
        if (ja < 0 || ja >= na) continue;
        if (MASK && (((g.dmask & (1 << (2 * A))) && ja == 0) || ((g.dmask & (2 << (2 * A))) && ja == na - 1))) continue;
        for (int kb = 0; kb < wb; ++kb) {
            const int jb = rb + kb - pb;
            if (jb < 0 || jb >= nb) continue;
            if (MASK && (((g.dmask & (1 << (2 * B))) && jb == 0) || ((g.dmask & (2 << (2 * B))) && jb == nb - 1))) continue;
            s = fma(Sr[ka * wb + kb], x[xo + (int64_t)(ja - ra) * st[A] + (int64_t)(jb - rb) * st[B]], s);
        }
    }
    return s;
}

template <int EPI, bool TENSOR, bool MASK, bool FACE>
__global__ void __launch_bounds__(256)
matfree_kernel(const MatfreeGeom g, const AssembleAxis A0, const AssembleAxis A1, const AssembleAxis A2,
               const double* __restrict__ x, double* __restrict__ y, const double* __restrict__ b,
               const double* __restrict__ a_q, const double* __restrict__ c_q, const double* __restrict__ diag,
               double mass_coef, double omega, double* __restrict__ partial, double* __restrict__ partial2,
               double beta, const MatfreeFaces F) {
    __shared__ double sX[(MF_PMAX + 1) * MF_WW];   // ring of x window planes
    __shared__ double sU[2 * MF_WW];               // B0 x, B0' x
    __shared__ double sT[3 * MF_QW];               // B1 U, B1 U', B1' U  at [q1][c2]
    __shared__ double sG[4 * 4 * MF_Q];            // per wave: w c u, w a d0u, w a d1u, w a d2u of one q1 row
    __shared__ double sH[3 * MF_Q * MF_D];         // axis-2 gathers at [q1][i2]
    __shared__ double sY[(MF_PMAX + 1) * MF_DD];   // ring of output planes, one column per thread
    // the tile's slices of the axis-1 and axis-2 tables: basis values and derivatives of
    // its points, their weights, and each point's first function relative to the window
    __shared__ double sB1[MF_Q * (MF_PMAX + 1) * 2], sB2[MF_Q * (MF_PMAX + 1) * 2];
    __shared__ double sW1[MF_Q], sW2[MF_Q];
    __shared__ int sO1[MF_Q], sO2[MF_Q];
    // stage D's gather table: value and derivative of the tile's axis-2 functions at its
    // points, [q2][column], zero outside a function's support
    __shared__ double sGB2[MF_Q * MF_D * 2];
    __shared__ double red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int p0 = A0.p, p1 = A1.p, p2 = A2.p;
    const int nq0 = A0.nq, nq1 = A1.nq, nq2 = A2.nq;
    const int64_t NQ1 = (int64_t)A1.nel * nq1, NQ2 = (int64_t)A2.nel * nq2;
    const int i1l = tid / MF_D, i2l = tid % MF_D;   // this thread's output column (tid < 64)
    const int wr = tid >> 4, wc = tid & 15;          // this thread's window entry (MF_W <= 16)
    const int darr = lane / MF_D, dil = lane % MF_D; // stage D: array and column of lanes 0..23
    // TENSOR: points per component plane, and the operator's dimension (a 2D operator
    // has the trivial axis 0, p = 0)
    const int64_t gs = TENSOR ? (int64_t)A0.nel * nq0 * NQ1 * NQ2 : 0;
    const int gdim = p0 > 0 ? 3 : 2;
    double nrm = 0.0, dot = 0.0;
    for (int64_t t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
        const int t2 = (int)(t % g.tiles2), t1 = (int)((t / g.tiles2) % g.tiles1);
        const int ch = (int)(t / ((int64_t)g.tiles2 * g.tiles1));
        const int i1lo = t1 * MF_D, i1hi = min(i1lo + MF_D, g.n1);
        const int i2lo = t2 * MF_D, i2hi = min(i2lo + MF_D, g.n2);
        const int z0 = ch * g.chunk, z1 = min(z0 + g.chunk, g.n0);
        const int E0lo = A0.es[z0], E0hi = A0.ee[z1 - 1];
        const int E1lo = A1.es[i1lo], E1hi = A1.ee[i1hi - 1];
        const int E2lo = A2.es[i2lo], E2hi = A2.ee[i2hi - 1];
        const int Q1 = (E1hi - E1lo + 1) * nq1, Q2 = (E2hi - E2lo + 1) * nq2;
        const int c1lo = A1.first[E1lo], w1 = A1.first[E1hi] + p1 + 1 - c1lo;
        const int c2lo = A2.first[E2lo], w2 = A2.first[E2hi] + p2 + 1 - c2lo;
        const bool inwin = wr < w1 && wc < w2;
        const int widx = wr * w2 + wc;
        const bool own = tid < MF_DD && i1lo + i1l < i1hi && i2lo + i2l < i2hi;
        // supports of this thread's functions in the tile's points: stage E (axis 1, the
        // thread's column) and stage D (axis 2, lanes 0..23)
        int q1a = 0, q1b = 0, ia1 = 0, q2a = 0, q2b = 0;
        if (own) {
            const int i1 = i1lo + i1l;
            q1a = (A1.es[i1] - E1lo) * nq1;
            q1b = (A1.ee[i1] - E1lo + 1) * nq1;
            ia1 = i1 - c1lo;
        }
        if (lane < 3 * MF_D && i2lo + dil < i2hi) {
            const int i2 = i2lo + dil;
            q2a = (A2.es[i2] - E2lo) * nq2;
            q2b = (A2.ee[i2] - E2lo + 1) * nq2;
        }
        __syncthreads();   // the previous tile's readers of the tables are done
        for (int k = tid; k < Q1 * (p1 + 1) * 2; k += 256) sB1[k] = A1.basis[(int64_t)E1lo * nq1 * (p1 + 1) * 2 + k];
        for (int k = tid; k < Q2 * (p2 + 1) * 2; k += 256) sB2[k] = A2.basis[(int64_t)E2lo * nq2 * (p2 + 1) * 2 + k];
        for (int k = tid; k < Q1; k += 256) {
            sW1[k] = A1.w[E1lo * nq1 + k];
            sO1[k] = A1.first[E1lo + k / nq1] - c1lo;
        }
        for (int k = tid; k < Q2; k += 256) {
            sW2[k] = A2.w[E2lo * nq2 + k];
            sO2[k] = A2.first[E2lo + k / nq2] - c2lo;
        }
        for (int k = tid; k < Q2 * MF_D; k += 256) {
            const int q2 = k / MF_D, il = k % MF_D, i2 = i2lo + il;
            const int a = i2 - A2.first[E2lo + q2 / nq2];
            const bool in = i2 < i2hi && a >= 0 && a <= p2;
            const double* B2 = A2.basis + ((int64_t)(E2lo * nq2 + q2) * (p2 + 1) + (in ? a : 0)) * 2;
            sGB2[2 * k] = in ? B2[0] : 0.0;
            sGB2[2 * k + 1] = in ? B2[1] : 0.0;
        }
        if (tid < MF_DD)
            for (int s = 0; s <= p0; ++s) sY[s * MF_DD + tid] = 0.0;
        int xnext = 0;    // x planes below it are in the ring (or no longer needed)
        int jf = z0;      // next output plane to finish
        for (int e0 = E0lo; e0 <= E0hi; ++e0) {
            const int f0 = A0.first[e0];
            __syncthreads();   // the tables are staged; the ring's readers of the previous element are done
            for (int j = max(xnext, f0); j <= f0 + p0; ++j)
                if (inwin)
                    sX[(j % (p0 + 1)) * MF_WW + widx] =
                        x[(int64_t)(j + g.pd0) * g.s0 + (int64_t)(c1lo + wr + g.pd1) * g.s1 + (c2lo + wc + g.pd2)];
            // Dirichlet faces: the constrained entries of the planes just loaded enter the
            // window as 0 (every thread zeroes what it wrote itself)
            if (MASK && inwin) {
                const int c1 = c1lo + wr, c2 = c2lo + wc;
                const bool fix12 = ((g.dmask & 4) && c1 == 0) || ((g.dmask & 8) && c1 == g.n1 - 1) ||
                                   ((g.dmask & 16) && c2 == 0) || ((g.dmask & 32) && c2 == g.n2 - 1);
                for (int j = max(xnext, f0); j <= f0 + p0; ++j)
                    if (fix12 || ((g.dmask & 1) && j == 0) || ((g.dmask & 2) && j == g.n0 - 1))
                        sX[(j % (p0 + 1)) * MF_WW + widx] = 0.0;
            }
            xnext = f0 + p0 + 1;
            __syncthreads();
            for (int q0 = 0; q0 < nq0; ++q0) {
                const int q0g = e0 * nq0 + q0;
                const double* B0 = A0.basis + (int64_t)q0g * (p0 + 1) * 2;
                const double wq0 = A0.w[q0g];
                const int64_t qrow = (int64_t)q0g * NQ1 + (int64_t)E1lo * nq1;
                // the coefficients of this wave's first row (each round fetches the next round's)
                double an = 1.0, cn = mass_coef;
                Tensor6 gn;
                if (wave < Q1 && lane < Q2) {
                    const int64_t qi = (qrow + wave) * NQ2 + (E2lo * nq2 + lane);
                    if constexpr (TENSOR) {
                        tensor_load(gn, a_q, qi, gs, gdim);
                    } else {
                        if (a_q) an = a_q[qi];
                    }
                    if (c_q) cn = c_q[qi];
                }
                // A: contract the p0+1 window planes with B0, B0'
                if (inwin) {
                    double u = 0.0, du = 0.0;
                    for (int a = 0; a <= p0; ++a) {
                        const double xv = sX[((f0 + a) % (p0 + 1)) * MF_WW + widx];
                        u = fma(B0[2 * a], xv, u);
                        du = fma(B0[2 * a + 1], xv, du);
                    }
                    sU[widx] = u;
                    sU[MF_WW + widx] = du;
                }
                __syncthreads();
                // B: expand along axis 1
                if (wc < w2)
                    for (int q1 = wr; q1 < Q1; q1 += 16) {
                        const int off = sO1[q1];
                        const double* B1 = sB1 + q1 * (p1 + 1) * 2;
                        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
                        for (int a = 0; a <= p1; ++a) {
                            const double uv = sU[(off + a) * w2 + wc], dv = sU[MF_WW + (off + a) * w2 + wc];
                            v0 = fma(B1[2 * a], uv, v0);
                            v1 = fma(B1[2 * a], dv, v1);
                            v2 = fma(B1[2 * a + 1], uv, v2);
                        }
                        sT[q1 * w2 + wc] = v0;
                        sT[MF_QW + q1 * w2 + wc] = v1;
                        sT[2 * MF_QW + q1 * w2 + wc] = v2;
                    }
                __syncthreads();
                // C, D: one wave per q1 row
                double* G = sG + wave * 4 * MF_Q;
                const int rounds = (Q1 + 3) / 4;
                for (int r = 0; r < rounds; ++r) {
                    const int q1 = r * 4 + wave;
                    const double ca = an, cc = cn;
                    const Tensor6 cg = gn;
                    if (q1 + 4 < Q1 && lane < Q2) {
                        const int64_t qi = (qrow + q1 + 4) * NQ2 + (E2lo * nq2 + lane);
                        if constexpr (TENSOR) {
                            tensor_load(gn, a_q, qi, gs, gdim);
                        } else {
                            if (a_q) an = a_q[qi];
                        }
                        if (c_q) cn = c_q[qi];
                    }
                    if (q1 < Q1 && lane < Q2) {
                        const double* B2 = sB2 + lane * (p2 + 1) * 2;
                        const double* T = sT + q1 * w2 + sO2[lane];
                        double u = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0;
                        for (int a = 0; a <= p2; ++a) {
                            const double bv = B2[2 * a], bd = B2[2 * a + 1], tv = T[a];
                            u = fma(bv, tv, u);
                            d2 = fma(bd, tv, d2);
                            d0 = fma(bv, T[MF_QW + a], d0);
                            d1 = fma(bv, T[2 * MF_QW + a], d1);
                        }
                        const double w = wq0 * (sW1[q1] * sW2[lane]);
                        const double wa = w * ca;
                        const double wc_ = w * cc;
                        G[lane] = wc_ * u;
                        if constexpr (TENSOR) {
                            G[MF_Q + lane] = w * fma(cg.g02, d2, fma(cg.g01, d1, cg.g00 * d0));
                            G[2 * MF_Q + lane] = w * fma(cg.g12, d2, fma(cg.g11, d1, cg.g01 * d0));
                            G[3 * MF_Q + lane] = w * fma(cg.g22, d2, fma(cg.g12, d1, cg.g02 * d0));
                        } else {
                            G[MF_Q + lane] = wa * d0;
                            G[2 * MF_Q + lane] = wa * d1;
                            G[3 * MF_Q + lane] = wa * d2;
                        }
                    }
                    __syncthreads();
                    // (G is the wave's own: its next round's stores follow these loads in
                    // program order)
                    // arrays 0, 1: B2 (w a d0u), B2 (w a d1u); array 2: B2 (w c u) + B2' (w a d2u)
                    // (one body for the three: the derivative term times 0 where it is not wanted)
                    if (q1 < Q1 && lane < 3 * MF_D) {
                        const double* ga = G + (darr == 0 ? MF_Q : darr == 1 ? 2 * MF_Q : 0);
                        const double* gb = G + 3 * MF_Q;
                        const double* tb = sGB2 + 2 * dil;
                        const double dsel = darr == 2 ? 1.0 : 0.0;
                        double s = 0.0;
#pragma unroll 4
                        for (int q2 = q2a; q2 < q2b; ++q2) {
                            s = fma(tb[2 * MF_D * q2], ga[q2], s);
                            s = fma(tb[2 * MF_D * q2 + 1] * dsel, gb[q2], s);
                        }
                        sH[(darr * MF_Q + q1) * MF_D + dil] = s;
                    }
                }
                __syncthreads();
                // E, F: gather along axis 1, add to the rolling output planes
                if (own) {
                    double v0 = 0.0, v1 = 0.0;
#pragma unroll 4
                    for (int q1 = q1a; q1 < q1b; ++q1) {
                        const double* B1 = sB1 + (q1 * (p1 + 1) + (ia1 - sO1[q1])) * 2;
                        v0 = fma(B1[0], sH[q1 * MF_D + i2l], v0);
                        v1 = fma(B1[1], sH[(MF_Q + q1) * MF_D + i2l], v1);
                        v1 = fma(B1[0], sH[(2 * MF_Q + q1) * MF_D + i2l], v1);
                    }
                    for (int a = 0; a <= p0; ++a) {
                        const int j = f0 + a;
                        if (j < z0 || j >= z1) continue;
                        double s = sY[(j % (p0 + 1)) * MF_DD + tid];
                        s = fma(B0[2 * a + 1], v0, s);
                        s = fma(B0[2 * a], v1, s);
                        sY[(j % (p0 + 1)) * MF_DD + tid] = s;
                    }
                }
            }
            // output planes whose last element this was
            while (jf < z1 && A0.ee[jf] <= e0) {
                if (own) {
                    const int i1 = i1lo + i1l, i2 = i2lo + i2l;
                    double s = sY[(jf % (p0 + 1)) * MF_DD + tid];
                    sY[(jf % (p0 + 1)) * MF_DD + tid] = 0.0;
                    const int64_t xo = (int64_t)(jf + g.pd0) * g.s0 + (int64_t)(i1 + g.pd1) * g.s1 + (i2 + g.pd2);
                    // face terms, in the order axis 0 lo, axis 0 hi, axis 1 lo, ...
                    if constexpr (FACE) {
                        if ((F.mask & 1) && jf == 0) s = face_row<0, MASK>(s, F.s[0], g, p1, p2, jf, i1, i2, x, xo);
                        if ((F.mask & 2) && jf == g.n0 - 1) s = face_row<0, MASK>(s, F.s[1], g, p1, p2, jf, i1, i2, x, xo);
                        if ((F.mask & 4) && i1 == 0) s = face_row<1, MASK>(s, F.s[2], g, p0, p2, jf, i1, i2, x, xo);
                        if ((F.mask & 8) && i1 == g.n1 - 1) s = face_row<1, MASK>(s, F.s[3], g, p0, p2, jf, i1, i2, x, xo);
                        if ((F.mask & 16) && i2 == 0) s = face_row<2, MASK>(s, F.s[4], g, p0, p1, jf, i1, i2, x, xo);
                        if ((F.mask & 32) && i2 == g.n2 - 1) s = face_row<2, MASK>(s, F.s[5], g, p0, p1, jf, i1, i2, x, xo);
                    }
                    // a constrained row applies its diagonal entry only
                    if (MASK && (((g.dmask & 1) && jf == 0) || ((g.dmask & 2) && jf == g.n0 - 1) ||
                                    ((g.dmask & 4) && i1 == 0) || ((g.dmask & 8) && i1 == g.n1 - 1) ||
                                    ((g.dmask & 16) && i2 == 0) || ((g.dmask & 32) && i2 == g.n2 - 1)))
                        s = diag[((int64_t)jf * g.n1 + i1) * g.n2 + i2] * x[xo];
                    if constexpr (EPI == EPI_APPLY) {
                        y[xo] = s;
                    } else if constexpr (EPI == EPI_RESID) {
                        y[xo] = b[xo] - s;
                    } else if constexpr (EPI == EPI_JACOBI) {
                        const double bv = b[xo];
                        const double dr = omega * (bv - s) / diag[((int64_t)jf * g.n1 + i1) * g.n2 + i2];
                        const double xn = x[xo] + dr;
                        y[xo] = xn;
                        nrm = fma(dr, dr, nrm);
                        dot = fma(xn, bv, dot);
                    } else if constexpr (EPI == EPI_CHEBY) {
                        // the general stencil's Chebyshev step: y holds x_{k-1} on entry, x_{k+1}
                        // on exit; beta == 0 selects, the old y is then not read
                        const double xv = x[xo];
                        const double dr = omega * (b[xo] - s) / diag[((int64_t)jf * g.n1 + i1) * g.n2 + i2];
                        const double mom = beta != 0.0 ? beta * (xv - y[xo]) : 0.0;
                        y[xo] = xv + mom + dr;
                    } else {   // EPI_APPLYDOT
                        y[xo] = s;
                        dot = fma(x[xo], s, dot);
                    }
                }
                ++jf;
            }
        }
    }
    if (partial) {
        const double s = block_sum_256(nrm, red);
        if (tid == 0) partial[blockIdx.x] = s;
        __syncthreads();
    }
    if (partial2) {
        const double s = block_sum_256(dot, red);
        if (tid == 0) partial2[blockIdx.x] = s;
    }
}

// diag[i] = sum_q w (c phi_i^2 + a |grad phi_i|^2): assemble_kernel's centre offset
// (stencil_general.hip; the same expression, per element the quadrature sum first),
// one thread per row, dense C order.  TENSOR: sum_q w (c phi_i^2 + grad phi_i^T G grad
// phi_i), a_q the component planes of an ndim-dimensional operator.
template <bool TENSOR>
__global__ void __launch_bounds__(256)
matfree_diag_kernel(const AssembleAxis A0, const AssembleAxis A1, const AssembleAxis A2,
                    const double* __restrict__ a_q, const double* __restrict__ c_q, double mass_coef,
                    double* __restrict__ diag, int ndim) {
    const int64_t total = (int64_t)A0.n * A1.n * A2.n;
    const int64_t lin = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (lin >= total) return;
    const int i2 = (int)(lin % A2.n), i1 = (int)((lin / A2.n) % A1.n), i0 = (int)(lin / ((int64_t)A2.n * A1.n));
    const int64_t NQ1 = (int64_t)A1.nel * A1.nq, NQ2 = (int64_t)A2.nel * A2.nq;
    const int64_t gs = (int64_t)A0.nel * A0.nq * NQ1 * NQ2;
    double tot = 0.0;
    for (int e0 = A0.es[i0]; e0 <= A0.ee[i0]; ++e0) {
        const int l0 = i0 - A0.first[e0];
        for (int e1 = A1.es[i1]; e1 <= A1.ee[i1]; ++e1) {
            const int l1 = i1 - A1.first[e1];
            for (int e2 = A2.es[i2]; e2 <= A2.ee[i2]; ++e2) {
                const int l2 = i2 - A2.first[e2];
                double v = 0.0;
                for (int q0 = 0; q0 < A0.nq; ++q0) {
                    const double* B0 = A0.basis + ((int64_t)(e0 * A0.nq + q0) * (A0.p + 1) + l0) * 2;
                    const double w0 = A0.w[e0 * A0.nq + q0], b0 = B0[0], d0 = B0[1];
                    for (int q1 = 0; q1 < A1.nq; ++q1) {
                        const double* B1 = A1.basis + ((int64_t)(e1 * A1.nq + q1) * (A1.p + 1) + l1) * 2;
                        const double w1 = A1.w[e1 * A1.nq + q1], b1 = B1[0], d1 = B1[1];
                        for (int q2 = 0; q2 < A2.nq; ++q2) {
                            const double* B2 = A2.basis + ((int64_t)(e2 * A2.nq + q2) * (A2.p + 1) + l2) * 2;
                            const double w2 = A2.w[e2 * A2.nq + q2], b2 = B2[0], d2 = B2[1];
                            const double i_0 = b0 * (b1 * b2);
                            const double gx = (d0 * (b1 * b2)) * (d0 * (b1 * b2));
                            const double gy = (b0 * (d1 * b2)) * (b0 * (d1 * b2));
                            const double gz = (b0 * (b1 * d2)) * (b0 * (b1 * d2));
                            const int64_t qi = ((int64_t)(e0 * A0.nq + q0) * NQ1 + (e1 * A1.nq + q1)) * NQ2 +
                                               (e2 * A2.nq + q2);
                            const double cc = c_q ? c_q[qi] : mass_coef;
                            if constexpr (TENSOR) {
                                Tensor6 t;
                                tensor_load(t, a_q, qi, gs, ndim);
                                const double e_0 = d0 * (b1 * b2), e_1 = b0 * (d1 * b2), e_2 = b0 * (b1 * d2);
                                const double form = tensor_form(t, e_0, e_1, e_2, e_0, e_1, e_2);
                                v = fma(cc * i_0 * i_0 + form, w0 * (w1 * w2), v);
                            } else {
                                const double ca = a_q ? a_q[qi] : 1.0;
                                v = fma(cc * i_0 * i_0 + ca * (gx + gy + gz), w0 * (w1 * w2), v);
                            }
                        }
                    }
                }
                tot += v;
            }
        }
    }
    diag[lin] = tot;
}

int matfree_diag_launch(const AssembleAxis* ax, const double* a_q, const double* c_q, double mass_coef, double* diag,
                        hipStream_t st, int tensor_ndim) {
    const int64_t total = (int64_t)ax[0].n * ax[1].n * ax[2].n;
    if (total == 0) return 0;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (tensor_ndim)
        hipLaunchKernelGGL(matfree_diag_kernel<true>, grid, dim3(256), 0, st, ax[0], ax[1], ax[2], a_q, c_q, mass_coef,
                           diag, tensor_ndim);
    else
        hipLaunchKernelGGL(matfree_diag_kernel<false>, grid, dim3(256), 0, st, ax[0], ax[1], ax[2], a_q, c_q,
                           mass_coef, diag, 0);
    return 0;
}

// The tensor builds run two workgroups per CU like the scalar ones (the LDS sets that):
// any number of registers up to 256 keeps that, scratch does not.  False, with a
// message, if a build reports scratch or the attributes cannot be read.
bool matfree_tensor_builds_ok(std::string* why) {
#define POMS_MF_BUILDS(E)                                                                                   \
    (const void*)matfree_kernel<E, true, false, false>, (const void*)matfree_kernel<E, true, true, false>,     \
    (const void*)matfree_kernel<E, true, false, true>, (const void*)matfree_kernel<E, true, true, true>
    const void* fns[20] = {POMS_MF_BUILDS(EPI_APPLY), POMS_MF_BUILDS(EPI_RESID), POMS_MF_BUILDS(EPI_JACOBI),
                           POMS_MF_BUILDS(EPI_APPLYDOT), POMS_MF_BUILDS(EPI_CHEBY)};
#undef POMS_MF_BUILDS
    for (int k = 0; k < 20; ++k) {
        hipFuncAttributes at{};
        if (hipFuncGetAttributes(&at, fns[k]) != hipSuccess) {
            (void)hipGetLastError();
            *why = "the attributes of the tensor kernel could not be read";
            return false;
        }
        if (at.localSizeBytes != 0 || at.numRegs > 256) {
            *why = "tensor kernel build " + std::to_string(k) + " uses " + std::to_string(at.localSizeBytes) +
                   " B of scratch and " + std::to_string(at.numRegs) + " registers (0 B and at most 256 allowed)";
            return false;
        }
    }
    return true;
}

// One workgroup per tile, at most max_blocks of them (the partials fit the scratch);
// a workgroup then takes every gridDim-th tile.
int matfree_launch(int epi, const MatfreeGeom& g, const AssembleAxis* ax, const double* x, double* y, const double* b,
                   const double* a_q, const double* c_q, const double* diag, double mass_coef, double omega,
                   double* partial, double* partial2, int max_blocks, hipStream_t st, int* nblk_out, bool tensor,
                   double beta, const MatfreeFaces* faces) {
    const int nb = (int)std::min<int64_t>(g.ntiles, max_blocks);
    *nblk_out = nb;
    if (nb <= 0) return 0;
    const bool face = faces && faces->mask;
    const MatfreeFaces F = face ? *faces : MatfreeFaces{};
#define POMS_MF_LAUNCH1(E, T, M, FC)                                                                          \
    hipLaunchKernelGGL((matfree_kernel<E, T, M, FC>), dim3(nb), dim3(256), 0, st, g, ax[0], ax[1], ax[2], x, y, b,  \
                       a_q, c_q, diag, mass_coef, omega, partial, partial2, beta, F)
#define POMS_MF_LAUNCH2(E, T, M)                                                                              \
    do {                                                                                                      \
        if (face) POMS_MF_LAUNCH1(E, T, M, true);                                                             \
        else POMS_MF_LAUNCH1(E, T, M, false);                                                                 \
    } while (0)
#define POMS_MF_LAUNCH(E)                                                                                     \
    do {                                                                                                      \
        if (tensor && g.dmask) POMS_MF_LAUNCH2(E, true, true);                                                \
        else if (tensor) POMS_MF_LAUNCH2(E, true, false);                                                     \
        else if (g.dmask) POMS_MF_LAUNCH2(E, false, true);                                                    \
        else POMS_MF_LAUNCH2(E, false, false);                                                                \
    } while (0)
    switch (epi) {
        case EPI_APPLY: POMS_MF_LAUNCH(EPI_APPLY); break;
        case EPI_RESID: POMS_MF_LAUNCH(EPI_RESID); break;
        case EPI_JACOBI: POMS_MF_LAUNCH(EPI_JACOBI); break;
        case EPI_APPLYDOT: POMS_MF_LAUNCH(EPI_APPLYDOT); break;
        case EPI_CHEBY: POMS_MF_LAUNCH(EPI_CHEBY); break;
        default:
            set_error("matrix-free operator: unsupported epilogue");
            return 1;
    }
#undef POMS_MF_LAUNCH
#undef POMS_MF_LAUNCH2
#undef POMS_MF_LAUNCH1
    return 0;
}

}  // namespace poms
