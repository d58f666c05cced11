// Fused Kronecker(-sum) operator, v3: axis-2 pass in registers via DPP lane
// shifts, one barrier per plane.
//
// Same operator / epilogues / axis-0 march as v1 and v2.  What changes:
//   * lanes of a wave are 64 consecutive columns of the tile INCLUDING the
//     2P halo columns (58 output columns per tile at P = 3); each wave loads
//     whole 512-B rows of x straight into VGPRs (coalesced, prefetched one
//     plane ahead) and forms the 2P shifted neighbours with v_mov_b32_dpp
//     wave_shr:1 / wave_shl:1 -- no x tile in LDS, no LDS reads, no barrier
//     for the axis-2 pass;
//   * the (a, b) = (M2 x, K2 x) rows go to a DOUBLE-BUFFERED 16-B-pair LDS
//     tile; the axis-1 pass reads it after the plane's single barrier, so the
//     next plane's axis-2 writes never race with this plane's axis-1 reads;
//   * axis-1 Toeplitz constants / LDS table and per-plane axis-0 scalar loads
//     as in v2; epilogue operands issued before the prefetch; stores of
//     invalid points dropped by the buffer range check (no branches around
//     memory operations: exact vmcnt counting).
// Preconditions: storage pads == P on every used axis (checked by the host).
#include "common.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"

#include <cstdlib>
#include <type_traits>

namespace poms {

template <int P, int R, int NW, bool IS3D, int FORM, int EPI, int PF, int MODE = 0, bool FLAT = false>
__global__ void __launch_bounds__(NW * 64, ((P <= 3 && NW <= 8 ? 2 : 1) * NW * 64) / 256)  // 16 waves/CU for P <= 3
kron_v3_kernel(const double* __restrict__ x, double* __restrict__ y,
               const double* __restrict__ bvec,
               const double* __restrict__ a0t, const double* __restrict__ b0t,
               const double* __restrict__ a1, const double* __restrict__ b1,
               const double* __restrict__ a2, const double* __restrict__ b2,
               double* __restrict__ partial, double* __restrict__ partial2,
               const double* __restrict__ rdiag0, const KronGeom g, const ToepConst tc,
               const double omega) {
    constexpr int W = 2 * P + 1;
    constexpr int NT = NW * 64;
    const int TO = g.tout;                     // output columns per tile
    constexpr int T1 = NW * R;
    constexpr int XR = T1 + 2 * P;
    constexpr int NRW = (XR + NW - 1) / NW;  // axis-2 rows per wave
    constexpr int XRP = XR;                  // rows of the LDS (a, b) tile
    constexpr bool SUM = (FORM == FORM_SUM);
    constexpr int NS = IS3D ? W : 1;
    typedef double d2 __attribute__((ext_vector_type(2)));

    // EPI_JACOBI0: the x planes are b; each loaded value becomes x1 = omega b / diag(A)
    // (sweep 1 from x0 = 0), and the epilogue is sweep 2 -- x2 from one pass over b
    constexpr bool J0 = (EPI == EPI_JACOBI0);
    constexpr bool JAC = (EPI == EPI_JACOBI) || J0;
    static_assert(!J0 || FLAT, "EPI_JACOBI0 is built for the whole-array kernel");
    constexpr bool APD = (EPI == EPI_APPLYDOT);     // apply + x.(Ax) (pcg's p.q)
    // T2 (the whole-array build): axis-2 band rows from the Toeplitz constants
    // (symmetric pair sums) in interior column tiles and from an LDS table in the
    // two boundary tiles -- no per-lane copy of the 2(2P+1) coefficients in VGPRs.
    // The freed registers pay for the per-plane 1/diag path; x_in is re-read
    // (L2) instead of kept in the LDS ring.
    constexpr bool T2 = false;   // measured slower (x_in re-read, LDS-table boundary tiles): kept for reference
    constexpr bool XRING = (JAC || APD) && IS3D && !T2;
    constexpr int NRING = P + 1;            // x planes kept for the Jacobi update
    // (2D: one plane, so one (a, b) tile -- the double buffer serves the 3D march)
    __shared__ d2 ab_[SUM ? (IS3D ? 2 : 1) * XRP * 64 : 1];
    // x of the tile's output rows for the last P+1 planes (the Jacobi epilogue's
    // x_in): re-reading it from HBM P planes later costs 8 B/DOF (L2-evicted)
    __shared__ double xring[XRING ? NRING * T1 * 64 : 1];
    __shared__ double as_[SUM ? 1 : (IS3D ? 2 : 1) * XRP * 64];
    __shared__ double c1a[T1 * W];
    __shared__ double c1b[SUM ? T1 * W : 1];
    __shared__ double red[NW];
    __shared__ double c2t[T2 ? 2 * W * 64 : 1];   // [a|b][k][lane] boundary-tile axis-2 rows

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int nblk = gridDim.x;
    int bid;
    {
        const int b = blockIdx.x, q = nblk >> 3, rr = nblk & 7, xcd = b & 7, k = b >> 3;
        bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + k;
    }
    const int t2 = bid % g.tiles2;
    bid /= g.tiles2;
    const int t1 = bid % g.tiles1;
    const int ch = bid / g.tiles1;
    const int c0 = t2 * TO;             // first output column of the tile
    const int r0 = t1 * T1;
    const int i2 = c0 - P + lane;       // this lane's column (may be a halo column)
    const bool col_ok = lane >= P && lane < P + TO && i2 < g.n2;

    constexpr int WC = T2 ? 1 : W;
    double ca2[WC], cb2[WC];
    double d2a, d2b;   // this lane's axis-2 band diagonal (F2a, F2b)
    {
        const int ic = min(max(i2, 0), g.n2 - 1);
        if constexpr (T2) {
            d2a = a2[ic * W + P];
            d2b = SUM ? b2[ic * W + P] : 0.0;
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                ca2[k] = a2[ic * W + k];
                cb2[k] = SUM ? b2[ic * W + k] : 0.0;
            }
            d2a = ca2[P];
            d2b = cb2[P];
        }
    }
    const bool fast2 = (c0 >= tc.lo2) && (min(c0 + TO, g.n2) <= tc.hi2);
    if (T2 && !fast2) {
        for (int e = tid; e < W * 64; e += NT) {
            const int k = e >> 6, l = e & 63;
            const int col = min(max(c0 - P + l, 0), g.n2 - 1);
            c2t[e] = a2[col * W + k];
            c2t[W * 64 + e] = SUM ? b2[col * W + k] : 0.0;
        }
    }
    const bool fast1 = (r0 >= tc.lo1) && (r0 + T1 <= tc.hi1);
    // all output points of the tile in the axis-1/2 Toeplitz interior: diag(A)
    // depends on the plane only, 1/diag comes from the host-built rdiag0 table
    const bool fast12 = T2 && rdiag0 != nullptr && fast1 && (c0 >= tc.lo2) && (min(c0 + TO, g.n2) <= tc.hi2);
    if (!fast1) {
        for (int e = tid; e < T1 * W; e += NT) {
            const int rl = e / W, k = e - rl * W;
            const int row = min(r0 + rl, g.n1 - 1);
            c1a[e] = a1[row * W + k];
            if constexpr (SUM) c1b[e] = b1[row * W + k];
        }
    }

    int z0 = 0, z1 = 1;
    if constexpr (IS3D) {
        chunk_planes(g, ch, z0, z1);
    }
    const int nplanes = IS3D ? (z1 - z0) + 2 * P : 1;
    const int nsp = g.n0 + 2 * g.pd0;

    // this wave's axis-2 rows: rr = wv + j*NW; storage (row, col) = (r0 + rr, c0 + lane)
    int xoff[NRW];
#pragma unroll
    for (int j = 0; j < NRW; ++j) {
        const int rr = wv + j * NW;
        xoff[j] = rr < XR ? ((r0 + rr) * (int)g.s1 + (c0 + lane)) * 8 : 0x7ffffff0;
    }
    double xr[PF][NRW];
    // FLAT: one resource per array for the whole launch (array < 2 GiB, checked by the
    // host); planes are addressed by the scalar offset -- no per-plane descriptor math
    const uint32_t arr_bytes = FLAT ? (uint32_t)((int64_t)nsp * g.s0 * 8) : 0u;
    const __amdgpu_buffer_rsrc_t rx_all = make_rsrc(x, arr_bytes);
    const __amdgpu_buffer_rsrc_t rb_all = make_rsrc(bvec, (EPI != EPI_APPLY && !APD) ? arr_bytes : 0u);
    const __amdgpu_buffer_rsrc_t ry_all = make_rsrc(y, arr_bytes);
    const uint32_t plane8 = (uint32_t)(g.s0 * 8);
    auto load_plane = [&](int jj, int xb) {
        const int sp = IS3D ? jj + g.pd0 : 0;
        const bool ok = (sp >= 0) && (sp < nsp);
        if constexpr (FLAT) {
            // out-of-range planes by voffset (soffset is outside the range check)
            const uint32_t so = ok ? (uint32_t)sp * plane8 : 0u;
#pragma unroll
            for (int j = 0; j < NRW; ++j) xr[xb][j] = bload_s(rx_all, ok ? xoff[j] : 0x7ffffff0, so);
            return;
        }
        const __amdgpu_buffer_rsrc_t rs =
            make_rsrc(x + (int64_t)(ok ? sp : 0) * g.s0, ok ? plane_bytes(nsp - sp, g.s0) : 0u);
#pragma unroll
        for (int j = 0; j < NRW; ++j) xr[xb][j] = MODE == 2 ? (double)(jj * 7 + j) * 1e-3 + (double)lane : bload(rs, xoff[j]);
    };

    double acc[R][NS];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[r][s] = 0.0;
    double nrm = 0.0, dotp = 0.0;

    const int obase = ((r0 + wv * R + g.pd1) * (int)g.s1 + (i2 + g.pd2)) * 8;
    const int rowstep = (int)g.s1 * 8;
    double ebb[PF][R], ex[R];
    // plane-invariant factors of diag(A) for row r of this thread (recomputed
    // per plane: cheaper than keeping 2R doubles live)
    auto diag_parts = [&](int r, double& dX, double& dY) {
        const double d1a = fast1 ? tc.t1a[0] : c1a[(wv * R + r) * W + P];
        const double d1b = SUM ? (fast1 ? tc.t1b[0] : c1b[(wv * R + r) * W + P]) : 0.0;
        if constexpr (IS3D) {
            dX = d1a * d2a;
            dY = SUM ? (d1b * d2a + d1a * d2b) : 0.0;
        } else {
            dX = SUM ? diag2d_sum(d1a, d2a, d1b, d2b) : d1a * d2a;
            dY = 0.0;
        }
    };
    auto epi_issue = [&](int zo, int eb_i) {
        double* eb = ebb[eb_i];
        if constexpr (APD && !XRING) {   // x at the output rows from memory (2D, or T2)
            const uint32_t so = FLAT ? (uint32_t)(zo + g.pd0) * plane8 : 0u;
            const __amdgpu_buffer_rsrc_t xsr = FLAT ? rx_all : make_rsrc(x + (int64_t)(zo + g.pd0) * g.s0,
                                                                         plane_bytes(nsp - zo - g.pd0, g.s0));
#pragma unroll
            for (int r = 0; r < R; ++r) ex[r] = bload_s(xsr, obase + r * rowstep, so);
        } else if constexpr (APD) {
        } else if constexpr (EPI != EPI_APPLY && FLAT) {
            const uint32_t so = (uint32_t)(zo + g.pd0) * plane8;
#pragma unroll
            for (int r = 0; r < R; ++r) eb[r] = bload_s(rb_all, obase + r * rowstep, so);
            if constexpr (JAC && !J0 && !XRING) {
#pragma unroll
                for (int r = 0; r < R; ++r) ex[r] = bload_s(rx_all, obase + r * rowstep, so);
            }
        } else if constexpr (EPI != EPI_APPLY) {
            const int sp = zo + g.pd0;
            const uint32_t nb = plane_bytes(nsp - sp, g.s0);
            const __amdgpu_buffer_rsrc_t bs = make_rsrc(bvec + (int64_t)sp * g.s0, nb);
#pragma unroll
            for (int r = 0; r < R; ++r) eb[r] = bload(bs, obase + r * rowstep);
            if constexpr (JAC && !XRING) {
                const __amdgpu_buffer_rsrc_t xsr = make_rsrc(x + (int64_t)sp * g.s0, nb);
#pragma unroll
                for (int r = 0; r < R; ++r) ex[r] = bload(xsr, obase + r * rowstep);
            }
        }
    };
    auto epi_finish = [&](int zo, const double* v, bool en, int eb_i) {
        const double* eb = ebb[eb_i];
        const int sp = zo + g.pd0;
        const __amdgpu_buffer_rsrc_t ys = make_rsrc(y + (int64_t)sp * g.s0, plane_bytes(nsp - sp, g.s0));
        double d0a = 1.0, d0b = 0.0;
        if constexpr (JAC && IS3D) {
            const int i0g = g.g0 + zo;
            d0a = a0t[(i0g + P) * W + P];
            if constexpr (SUM) d0b = b0t[(i0g + P) * W + P];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool ok = en && col_ok && (r0 + wv * R + r < g.n1);
            double outv;
            if constexpr (EPI == EPI_APPLY) {
                outv = v[r];
            } else if constexpr (APD) {
                outv = v[r];
                dotp = ok ? fma(ex[r], outv, dotp) : dotp;
            } else if constexpr (EPI == EPI_RESID) {
                outv = eb[r] - v[r];
            } else {
                double rc;
                if (fast12) {
                    rc = rdiag0[IS3D ? g.g0 + zo : 0];
                } else {
                    double dX, dY;
                    diag_parts(r, dX, dY);
                    const double diag = IS3D ? fma(d0a, dX, d0b * dY) : dX;
                    rc = __builtin_amdgcn_rcp(diag);
                    double e = fma(-diag, rc, 1.0);
                    rc = fma(rc, e, rc);
                    e = fma(-diag, rc, 1.0);
                    rc = fma(rc, e, rc);
                }
                if constexpr (J0 && !XRING) ex[r] = omega * eb[r] * rc;   // x1 at the output point
                const double dr = omega * (eb[r] - v[r]) * rc;
                if constexpr (IS3D) outv = ex[r] + dr;
                else outv = add_nc(ex[r], dr);   // (kron2d_j2_kernel's bits)
                nrm = ok ? fma(dr, dr, nrm) : nrm;
                if constexpr (J0) dotp = ok ? fma(ex[r], ex[r], dotp) : dotp;   // ||x1||^2 = ||dr_1||^2
                else dotp = ok ? fma(outv, eb[r], dotp) : dotp;                  // x_out . b (pcg's s.r)
            }
            if constexpr (MODE == 2) {
                if (outv == 12345.678) bstore(ys, ok ? obase + r * rowstep : 0x7ffffff0, outv);
            } else if constexpr (FLAT) {
                bstore_s(ry_all, ok ? obase + r * rowstep : 0x7ffffff0, (uint32_t)sp * plane8, outv);
            } else {
                bstore(ys, ok ? obase + r * rowstep : 0x7ffffff0, outv);
            }
        }
    };

    auto zo_of = [&](int t) { return IS3D ? max(z0 - 2 * P + t, z0) : 0; };
    load_plane(IS3D ? z0 - P : 0, 0);
    if constexpr (PF == 2) {
        load_plane(IS3D ? (1 < nplanes ? z0 - P + 1 : -(1 << 20)) : 0, 1);
        epi_issue(zo_of(0), 0);
    }
    __syncthreads();  // c1a/c1b visible

    for (int tb = 0; tb < nplanes; tb += NS * PF) {
#pragma unroll
        for (int q2 = 0; q2 < NS * PF; ++q2) {
            const int t = tb + q2;
            const int q = q2 % NS;
            const int xb = q2 % PF;
            if (t < nplanes) {
                const int buf = IS3D ? (t & 1) * XRP * 64 : 0;
                // ---- axis 2 in registers: DPP shifts of whole rows
#pragma unroll
                for (int j = 0; j < NRW; ++j) {
                    double sh[W];
                    sh[P] = xr[xb][j];
                    if constexpr (J0) {
                        // x1 = (omega b) / diag(A) at (plane m, row, column) -- the
                        // diag_scale kernel's expression; clamped indices keep diag
                        // finite where b is a zero ghost.  2D (round 6): diag = d1a d2a +
                        // d1b d2b, the epilogue's diag_parts expression, so that x1 at a
                        // stencil input and at the output point are the same bits
                        const int row = min(max(r0 - P + wv + j * NW, 0), g.n1 - 1);
                        const double q1a = a1[row * W + P];
                        const double q1b = SUM ? b1[row * W + P] : 0.0;
                        double dg;
                        if constexpr (IS3D) {
                            const int m = g.g0 + z0 - P + t;
                            const int mc = min(max(m, 0), g.g0 + g.n0 + g.pd0 - 1);
                            const double q0a = a0t[(mc + P) * W + P];
                            const double q0b = SUM ? b0t[(mc + P) * W + P] : 0.0;
                            dg = SUM ? q0a * (q1a * d2a) + q0b * (q1b * d2a + q1a * d2b) : q0a * q1a * d2a;
                        } else {
                            // (the row's own band entries: a halo row of a fast1 tile may lie
                            // outside the Toeplitz interior; inside it they equal tc.t1a/t1b[0]
                            // bitwise, which the epilogue uses for the output rows)
                            dg = SUM ? diag2d_sum(q1a, d2a, q1b, d2b) : q1a * d2a;
                        }
                        double rc = __builtin_amdgcn_rcp(dg);
                        double e = fma(-dg, rc, 1.0);
                        rc = fma(rc, e, rc);
                        e = fma(-dg, rc, 1.0);
                        rc = fma(rc, e, rc);
                        rc = dg != 0.0 ? rc : 0.0;
                        sh[P] = omega * sh[P] * rc;
                    }
#pragma unroll
                    for (int d = 1; d <= P; ++d) {
                        sh[P - d] = shr1(sh[P - d + 1]);  // column i2 - d
                        sh[P + d] = shl1(sh[P + d - 1]);  // column i2 + d
                    }
                    double sa, sb = 0.0;
                    if constexpr (MODE == 1) {
                        sa = xr[xb][j];
                        sb = sa;
                    } else if constexpr (!T2) {
                        sa = ca2[0] * sh[0];
                        sb = SUM ? cb2[0] * sh[0] : 0.0;
#pragma unroll
                        for (int k = 1; k < W; ++k) {
                            sa = fma(ca2[k], sh[k], sa);
                            if constexpr (SUM) sb = fma(cb2[k], sh[k], sb);
                        }
                    } else if (fast2) {
                        // symmetric Toeplitz interior: P pair sums, P + 1 multiplies per product
                        double pr2[P + 1];
                        pr2[0] = sh[P];
#pragma unroll
                        for (int k = 1; k <= P; ++k) pr2[k] = sh[P - k] + sh[P + k];
                        sa = tc.t2a[0] * pr2[0];
                        if constexpr (SUM) sb = tc.t2b[0] * pr2[0];
#pragma unroll
                        for (int k = 1; k <= P; ++k) {
                            sa = fma(tc.t2a[k], pr2[k], sa);
                            if constexpr (SUM) sb = fma(tc.t2b[k], pr2[k], sb);
                        }
                    } else {
                        sa = c2t[lane] * sh[0];
                        if constexpr (SUM) sb = c2t[W * 64 + lane] * sh[0];
#pragma unroll
                        for (int k = 1; k < W; ++k) {
                            sa = fma(c2t[k * 64 + lane], sh[k], sa);
                            if constexpr (SUM) sb = fma(c2t[(W + k) * 64 + lane], sh[k], sb);
                        }
                    }
                    const int rr = wv + j * NW;
                    if constexpr (XRING) {
                        const int orow = rr - P;   // output row of this tile row, if any
                        if (orow >= 0 && orow < T1)
                            xring[(((t + NRING) % NRING) * T1 + orow) * 64 + lane] = sh[P];
                    }
                    if (XR % NW == 0 || rr < XR) {
                        if constexpr (SUM) {
                            d2 pr;
                            pr.x = sa;
                            pr.y = sb;
                            ab_[buf + rr * 64 + lane] = pr;
                        } else {
                            as_[buf + rr * 64 + lane] = sa;
                        }
                    }
                }
                // ---- loads for the rest of the iteration / the next plane
                if constexpr (PF == 1) epi_issue(zo_of(t), 0);
                else epi_issue(zo_of(t + 1), (q2 + 1) % PF);
                if constexpr (XRING) {
                    // x_in of this iteration's output plane (input plane t-P): read
                    // BEFORE the barrier -- its slot is rewritten by iteration t+1's
                    // axis-2 pass, which runs after this barrier.
                    const int slot = (t - P + NRING) % NRING;
#pragma unroll
                    for (int r = 0; r < R; ++r) ex[r] = xring[(slot * T1 + wv * R + r) * 64 + lane];
                }
                if constexpr (IS3D) load_plane(t + PF < nplanes ? z0 - P + t + PF : -(1 << 20), xb);
                __syncthreads();

                // ---- axis 1 from the LDS tile
                double cv[R], dv[R];
#pragma unroll
                for (int r = 0; r < R; ++r) { cv[r] = 0.0; dv[r] = 0.0; }
                auto axis1 = [&](auto coef) {
#pragma unroll
                    for (int qq = 0; qq < R + 2 * P; ++qq) {
                        const int rr = wv * R + qq;
                        double va, vb = 0.0;
                        if constexpr (SUM) {
                            const d2 pr = ab_[buf + rr * 64 + lane];
                            va = pr.x;
                            vb = pr.y;
                        } else {
                            va = as_[buf + rr * 64 + lane];
                        }
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const int k = qq - r;
                            if (k >= 0 && k < W) {
                                double ca, cb;
                                coef(r, k, ca, cb);
                                cv[r] = fma(ca, va, cv[r]);
                                if constexpr (SUM) {
                                    if constexpr (IS3D) dv[r] = fma(cb, va, fma(ca, vb, dv[r]));
                                    else cv[r] = fma(cb, vb, cv[r]);
                                }
                            }
                        }
                    }
                };
                if constexpr (MODE == 1) {
                    const d2 pr = ab_[buf + (wv * R + P) * 64 + lane];
                    for (int r = 0; r < R; ++r) { cv[r] = pr.x; dv[r] = pr.y; }
                } else if (fast1) {
                    axis1([&](int, int k, double& ca, double& cb) {
                        const int jj = k < P ? P - k : k - P;
                        ca = tc.t1a[jj];
                        cb = SUM ? tc.t1b[jj] : 0.0;
                    });
                } else {
                    axis1([&](int r, int k, double& ca, double& cb) {
                        ca = c1a[(wv * R + r) * W + k];
                        cb = SUM ? c1b[(wv * R + r) * W + k] : 0.0;
                    });
                }

                if constexpr (IS3D && MODE == 1) {
                    double vv[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) vv[r] = cv[r] + dv[r];
                    epi_finish(zo_of(t), vv, t >= 2 * P, PF == 1 ? 0 : xb);
                } else if constexpr (IS3D) {
                    // ---- axis 0: scatter into rotating slots
                    const int jrow = (g.g0 + z0 - P + t + P) * W;
#pragma unroll
                    for (int s = 0; s < W; ++s) {
                        const int slot = (q - P + s + NS) % NS;
                        const double ka = a0t[jrow + s];
                        const double kb = SUM ? b0t[jrow + s] : 0.0;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            acc[r][slot] = fma(ka, cv[r], acc[r][slot]);
                            if constexpr (SUM) acc[r][slot] = fma(kb, dv[r], acc[r][slot]);
                        }
                    }
                    const int done = (q + P + 1) % NS;
                    double vv[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) vv[r] = acc[r][done];
                    epi_finish(zo_of(t), vv, t >= 2 * P, PF == 1 ? 0 : xb);
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r][done] = 0.0;
                } else {
                    epi_finish(0, cv, true, 0);
                }
            }
        }
    }

    if constexpr (JAC || APD) {
        if (partial != nullptr) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) nrm += __shfl_xor(nrm, off, 64);
            if (lane == 0) red[wv] = nrm;
            __syncthreads();
            if (tid == 0) {
                double s = 0.0;
                for (int w = 0; w < NW; ++w) s += red[w];
                partial[blockIdx.x] = s;
            }
        }
        if (partial2 != nullptr) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) dotp += __shfl_xor(dotp, off, 64);
            __syncthreads();
            if (lane == 0) red[wv] = dotp;
            __syncthreads();
            if (tid == 0) {
                double s = 0.0;
                for (int w = 0; w < NW; ++w) s += red[w];
                partial2[blockIdx.x] = s;
            }
        }
    }
}

template <int P, int R, int NW, bool IS3D, int FORM, int EPI, int PF, int MODE = 0, bool FLAT = false>
static void v3_launch_t(const KronPtrs& p, const KronGeom& g, const ToepConst& tc, double omega,
                        hipStream_t st) {
    const int nblk = g.tiles2 * g.tiles1 * g.nchunks;
    hipLaunchKernelGGL((kron_v3_kernel<P, R, NW, IS3D, FORM, EPI, PF, MODE, FLAT>), dim3(nblk), dim3(NW * 64), 0, st,
                       p.x, p.y, p.b, p.a0t, p.b0t, p.a1, p.b1, p.a2, p.b2, p.partial, p.partial2, p.rdiag0, g, tc, omega);
}

template <int P, int R, int NW, bool IS3D, int FORM, int PF, bool FLAT = false>
static int v3_launch_e(int epi, const KronPtrs& p, const KronGeom& g, const ToepConst& tc,
                       double omega, hipStream_t st) {
    if (epi == EPI_APPLYDOT) {
        v3_launch_t<P, R, NW, IS3D, FORM, EPI_APPLYDOT, PF, 0, FLAT>(p, g, tc, omega, st);
        return 0;
    }
    if (epi == EPI_JACOBI0) {
        if constexpr (FLAT) {
            v3_launch_t<P, R, NW, IS3D, FORM, EPI_JACOBI0, PF, 0, FLAT>(p, g, tc, omega, st);
            return 0;
        }
        set_error("two sweeps from zero: the whole-array kernel (variant 8/9) only");
        return 1;
    }
    switch (epi) {
        case EPI_APPLY: v3_launch_t<P, R, NW, IS3D, FORM, EPI_APPLY, PF, 0, FLAT>(p, g, tc, omega, st); return 0;
        case EPI_RESID: v3_launch_t<P, R, NW, IS3D, FORM, EPI_RESID, PF, 0, FLAT>(p, g, tc, omega, st); return 0;
        case EPI_JACOBI: v3_launch_t<P, R, NW, IS3D, FORM, EPI_JACOBI, PF, 0, FLAT>(p, g, tc, omega, st); return 0;
    }
    return 1;
}

template <int P, int R, int NW, int PF = 1, bool FLAT = false>
static int v3_launch_p(bool is3d, int form, int epi, const KronPtrs& p, const KronGeom& g,
                       const ToepConst& tc, double omega, hipStream_t st) {
    if (is3d)
        return form == FORM_SUM ? v3_launch_e<P, R, NW, true, FORM_SUM, PF, FLAT>(epi, p, g, tc, omega, st)
                                : v3_launch_e<P, R, NW, true, FORM_SINGLE, PF, FLAT>(epi, p, g, tc, omega, st);
    return form == FORM_SUM ? v3_launch_e<P, R, NW, false, FORM_SUM, PF, FLAT>(epi, p, g, tc, omega, st)
                            : v3_launch_e<P, R, NW, false, FORM_SINGLE, PF, FLAT>(epi, p, g, tc, omega, st);
}

// Output rows per tile of the 2D p = 3 whole-array build (variant 9): 8 waves x R rows.
// R = 5 (40-row tiles): at 1024^2 the grid is 26 x 18 = 468 workgroups, one round of the
// 512 slots (2 per CU), against 1170 (2.3 rounds) for R = 2, and the host adds 468
// instead of 1170 norm partials per sweep; the 2D cycle 3.17 -> 2.90 ms, interleaved on
// one box (profiles/r06/r2d/; R = 3, 4, 6 between the two).  POMS_V3_2D_R overrides.
int kron_v3_rows_2d() {
    static int r = -1;
    if (r < 0) {
        const char* e = getenv("POMS_V3_2D_R");
        r = e ? atoi(e) : 5;
        if (r < 2 || r > 6) r = 2;
    }
    return 8 * r;
}

// variant 4: 8 waves x 2 rows (16 x (64-2P) tile, 2 WGs/CU); variant 9: the same
// tile addressing each array through one buffer resource
int kron_v3_launch(int variant, int pmax, bool is3d, int form, int epi, const KronPtrs& p,
                   const KronGeom& g, const ToepConst& tc, double omega, hipStream_t st) {
    if (variant == 90 || variant == 91) {   // DIAGNOSTIC: memory-only / compute-only apply, 3D SUM P=3
        if (pmax != 3 || !is3d || form != FORM_SUM || epi != EPI_APPLY) { set_error("diag variant: 3D SUM P=3 apply only"); return 1; }
        if (variant == 90) v3_launch_t<3, 2, 8, true, FORM_SUM, EPI_APPLY, 1, 1>(p, g, tc, omega, st);
        else v3_launch_t<3, 2, 8, true, FORM_SUM, EPI_APPLY, 1, 2>(p, g, tc, omega, st);
        return 0;
    }
    if (variant == 9) {   // v3 with whole-array buffer resources (arrays < 2 GiB)
        const int64_t bytes = (int64_t)(g.n0 + 2 * g.pd0) * g.s0 * 8;
        // 2D at p = 3: taller tiles (R rows per wave, kron_v3_rows_2d) so that the grid
        // is about one round of the CUs (tuning: POMS_V3_2D_R)
        if (!is3d && pmax == 3 && bytes < 0x7ffffff0LL) {
            auto l2 = [&](auto rt) {
                constexpr int RR = decltype(rt)::value;
                return form == FORM_SUM ? v3_launch_e<3, RR, 8, false, FORM_SUM, 1, true>(epi, p, g, tc, omega, st)
                                        : v3_launch_e<3, RR, 8, false, FORM_SINGLE, 1, true>(epi, p, g, tc, omega, st);
            };
            switch (kron_v3_rows_2d() / 8) {
                case 3: return l2(std::integral_constant<int, 3>{});
                case 4: return l2(std::integral_constant<int, 4>{});
                case 5: return l2(std::integral_constant<int, 5>{});
                case 6: return l2(std::integral_constant<int, 6>{});
                default: break;
            }
        }
        if (bytes < 0x7ffffff0LL) {
            switch (pmax) {
                case 1: return v3_launch_p<1, 2, 8, 1, true>(is3d, form, epi, p, g, tc, omega, st);
                case 2: return v3_launch_p<2, 2, 8, 1, true>(is3d, form, epi, p, g, tc, omega, st);
                case 3: return v3_launch_p<3, 2, 8, 1, true>(is3d, form, epi, p, g, tc, omega, st);
                case 4: return v3_launch_p<4, 2, 8, 1, true>(is3d, form, epi, p, g, tc, omega, st);
                case 5: return v3_launch_p<5, 2, 8, 1, true>(is3d, form, epi, p, g, tc, omega, st);
            }
        }
    }
    switch (pmax) {
        case 1: return v3_launch_p<1, 2, 8>(is3d, form, epi, p, g, tc, omega, st);
        case 2: return v3_launch_p<2, 2, 8>(is3d, form, epi, p, g, tc, omega, st);
        case 3: return v3_launch_p<3, 2, 8>(is3d, form, epi, p, g, tc, omega, st);
        case 4: return v3_launch_p<4, 2, 8>(is3d, form, epi, p, g, tc, omega, st);
        case 5: return v3_launch_p<5, 2, 8>(is3d, form, epi, p, g, tc, omega, st);
    }
    set_error("pmax must be in 1..5");
    return 1;
}

}  // namespace poms
