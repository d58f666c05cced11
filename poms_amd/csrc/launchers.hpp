// Host-side launchers of the kernel files, declared once: every file that defines one
// and every file that calls one includes this header (default arguments live here only).
#pragma once
#include "common.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace poms {

// ---- kron_fused.hip (v0), kron_dpp.hip (v3), kron_v4.hip, kron_v5.hip, kron_2d.hip ----
// (v5: kron_v5.hip is the host side; its kernel builds are compiled by kron_v5_p1.hip ..
// kron_v5_p5.hip and kron_v5_diag.hip from kron_v5_kernel.hpp, which declares those units'
// entries; kron_v5_stamps is defined in kron_v5_diag.hip beside the stamp buffer)
int kron_launch(int pmax, bool is3d, int form, int epi, const KronPtrs& p, const KronGeom& g,
                double omega, hipStream_t st);
int kron_tile_rows();
int kron_tile_cols();
int kron_v3_launch(int variant, int pmax, bool is3d, int form, int epi, const KronPtrs& p,
                   const KronGeom& g, const ToepConst& tc, double omega, hipStream_t st);
int kron_v3_rows_2d();
int kron_v4_launch(int pmax, bool is3d, int form, int epi, const KronPtrs& p, const KronGeom& g,
                   const ToepConst& tc, double omega, hipStream_t st, int diag_mode);
int kron_v5_launch(int pmax, int epi, const KronPtrs& p, const KronGeom& g, const ToepConst& tc, int H,
                   double omega, hipStream_t st, int diag_mode);
void kron_v5_tile(int pmax, bool aligned, int* H, int* TO);
int kron_v5_rows(int pmax, int epi, int same12);
int kron_v5_stamps(unsigned long long* host, int64_t n);
int kron_v5_set_sched(int mode);
void kron_v5_set_launch_events(hipEvent_t e0, hipEvent_t e1);
bool kron_v5_launch_events_used();
int kron2d_j2_rows();
int kron2d_j2_rows_default();
int kron2d_j2_cols(int pmax);
int kron2d_j2_launch(int pmax, int form, const KronPtrs& p, const KronGeom& g, const ToepConst& tc, double omega,
                     hipStream_t st, bool from_zero, double* part0);

// ---- vec_ops.hip ------------------------------------------------------------------
enum VecOp : int { V_AXPBY = 0, V_SCALE = 1, V_FILL = 2, V_DOT = 3, V_PCGUPD = 4, V_RUPD = 5, V_XPUPD = 6,
                  V_SCALEDOT = 7 /* z = a x and z.z (flat kernel only) */,
                  V_FINUPD = 8 /* pcg's last iteration, see stop_update */,
                  // pcg's deferred x updates (flat kernel only; pcg_native.hip)
                  V_PUPD = 9 /* z = x + b y: V_XPUPD's p into another buffer, its x untouched */,
                  V_RNORM = 10 /* V_RUPD's r.r without the store of r */,
                  V_SQNORM = 11 /* w.w with V_RUPD's grid, per-thread order and partials: on a stored
                                   r - a q the bits of V_RUPD's sum */ };

int vec_launch(int op, const RowGeom& g, double a, double b, const double* x, const double* y,
               double* z, double* w, const double* q, double* partial, hipStream_t st,
               int* nblk_out, const double* ab = nullptr);
int vec_flat_launch(int op, int64_t count, double a, double b, const double* x, const double* y,
                    double* z, double* w, const double* q, double* partial, hipStream_t st,
                    int* nblk_out, const double* ab = nullptr, const AlphaFold* af = nullptr);
// The range the flat kernels run over: a padded vector's whole interior planes, `count`
// doubles from `off` (ghost rows / columns inside it are zero in every vector).
struct FlatRange { int64_t off, count; };
inline FlatRange flat_range(const RowGeom& g) { return {(int64_t)g.pd0 * g.s0, (int64_t)g.n0 * g.s0}; }
// vec_flat_launch's grid over `count` doubles at `p`, before its cap (POMS_VEC_BLOCKS): a
// head double where p is off its 16-B phase, then 1024 pairs per block.  Callers that
// size a partials region or a fold by the grid take it from here.
inline int64_t vec_flat_blocks(int64_t count, const void* p) {
    const int head = (reinterpret_cast<uintptr_t>(p) & 15) ? 1 : 0;
    return std::max<int64_t>(1, ((count - head) / 2 + 256 * 4 - 1) / (256 * 4));
}
// x = fma(alpha[j], p_j, x) over `count` doubles for the n terms of `xa` (flat only; 1: the
// pointers do not share their 16-B phase, nothing launched)
int vec_xpass_launch(int64_t count, const XPassArgs& xa, const double* alpha, double* x, hipStream_t st);
int zero_ghosts_launch(const RowGeom& g, double* z, hipStream_t st);
int reduce_launch(const double* partial, int count, double* out, hipStream_t st, int accumulate = 0);
int reduce_wide_launch(const double* partial, int count, double* out, hipStream_t st, int accumulate = 0);
int diag_scale_blocks(bool is3d, const RowGeom& g);
int diag_scale_launch(bool is3d, int form, const RowGeom& g, int P, int g0, double scale,
                      const double* b, double* x, const double* a0t, const double* b0t,
                      const double* a1, const double* b1, const double* a2, const double* b2,
                      double* partial, hipStream_t st, int* nblk_out);
int dense_matvec_launch(int n, const double* M, const double* x, double* y, hipStream_t st);

// ---- block_ops.hip ----------------------------------------------------------------
// Lists of vectors over `count` doubles from each pointer (a flat range): the pointers go
// to the kernels by value, at most kBlockMax (POMS_BLOCK_MAX) of them per list.
constexpr int kBlockMax = 24;
constexpr int kCombineMaxOut = 16;
constexpr int kGramTile = 4;   // the Gram kernel's register tile: 4 x 4 sums per thread
constexpr int kGramMaxTiles = (kBlockMax / kGramTile) * (kBlockMax / kGramTile);
// out[i * ny + j] = x_i . y_j (symmetric: tiles on or above the diagonal only, the strict
// lower triangle copied from the upper); per-block partials in `partial` (kScratch doubles),
// then an ordered reduction.  1: a bad count or size, nothing launched.
int block_gram_launch(int64_t count, int nx, const double* const* xs, int ny, const double* const* ys,
                      int symmetric, double* partial, double* out, hipStream_t st);
// out_j = sum_i coef[i * nout + j] in_i (coef on the device); nin <= kBlockMax, nout <= kCombineMaxOut
int block_combine_launch(int64_t count, int nin, const double* const* ins, int nout, double* const* outs,
                         const double* coef, hipStream_t st);

// ---- stencil_general.hip ----------------------------------------------------------
// (tensor_ndim = 2 or 3: a_q holds the component planes of a tensor coefficient, see
// common.hpp's Tensor6; 0: a scalar field or null)
int assemble_launch(const AssembleAxis* ax, int g0, int nl0, const double* a_q, const double* c_q, double mass_coef,
                    double* coef, hipStream_t st, int tensor_ndim = 0);
int stencil_to_spl_launch(const StencilGeom& g, const double* coef, double* out, hipStream_t st);
// A face stencil [m_a][m_b][2 p_a + 1][2 p_b + 1] (the face's two axes in increasing order) added
// into the rows of the boundary plane `side` of `axis`: into the coefficient planes `coef` at the
// offsets (k_a, centre, k_b), or (diag not null) its centres into the dense diagonal `diag`.
int face_add_launch(const StencilGeom& g, int axis, int side, const double* face, double* coef, double* diag,
                    hipStream_t st);
int stencil_launch(int epi, const StencilGeom& g, const double* coef, const double* x, double* y,
                   const double* b, double omega, double* partial, double* partial2, int max_blocks,
                   hipStream_t st, int* nblk_out, double beta = 0.0);   // (beta: EPI_CHEBY only)

// ---- matfree.hip ------------------------------------------------------------------
int matfree_tile();           // output columns per tile edge (axes 1, 2)
int matfree_max_window();     // widest x window a tile may need per axis
int matfree_max_elements();   // most elements a tile may touch per axis
// (tensor / tensor_ndim as assemble_launch's: a_q is then the tensor's component planes)
int matfree_diag_launch(const AssembleAxis* ax, const double* a_q, const double* c_q, double mass_coef, double* diag,
                        hipStream_t st, int tensor_ndim = 0);
int matfree_launch(int epi, const MatfreeGeom& g, const AssembleAxis* ax, const double* x, double* y, const double* b,
                   const double* a_q, const double* c_q, const double* diag, double mass_coef, double omega,
                   double* partial, double* partial2, int max_blocks, hipStream_t st, int* nblk_out,
                   bool tensor = false, double beta = 0.0,    // (beta: EPI_CHEBY only)
                   const MatfreeFaces* faces = nullptr);     // (face terms: the FACE builds, or null)
bool matfree_tensor_builds_ok(std::string* why);   // no scratch, at most 256 registers

// ---- stencil_galerkin.hip ---------------------------------------------------------
// One axis of the Galerkin product P^T A P of a general stencil: coefficient planes
// [k0][k1][k2] of rows nin -> nout (they differ on axis d only).  Column I of P_d has
// its non-zero rows in [lo[I], lo[I] + cnt[I]); wt (device, smax * w[d]^2 doubles per
// column) holds the products P_d[i, I] P_d[i + k - p, I + kc - p]: a column's entries
// contiguous for the axis-0 and axis-1 passes (ws_ent = 1), the columns contiguous for
// the axis-2 pass, whose lanes differ in I (ws_col = 1).
struct GalerkinPass {
    int d;
    int w[3];
    int nin[3], nout[3];
    int smax;
    int64_t cst_in, cst_out;   // rows per plane
    int64_t ws_col, ws_ent;    // weight of (column I, entry e = (ii w + k) w + kc) at wt[I ws_col + e ws_ent]
    const int* lo;
    const int* cnt;
    const double* wt;
};

int galerkin_pass_launch(const GalerkinPass& g, const double* in, double* out, hipStream_t st);

// ---- transfer.hip -----------------------------------------------------------------
int transfer_pass_launch(bool restrict_dir, int ncm, const AxisPass& ps, const double* Pm,
                         const double* in, double* out, hipStream_t st, double* part);
int transfer_split_scratch(int ncm, const AxisPass& ps);
int transfer_band_launch(bool restrict_dir, const AxisPass& ps, const double* band, const int* lo, int w,
                         const double* in, double* out, hipStream_t st);

// One pass of the fused residual -> restriction: up to 3 inputs and 3 outputs
// sharing one AxisPass geometry; m[o][k] (device, rows padded to the pass's ncm
// columns, null = no term) maps input k into output o.
struct MultiPass {
    AxisPass ps;
    const double* in[3];
    double* out[3];
    const double* m[3][3];
    int ni, no;
};

int mrestrict_launch(int ncm, const MultiPass& mp, double* part, hipStream_t st);
int64_t mrestrict_scratch(const MultiPass& mp, int ncm);

// ---- kron_solve.hip ---------------------------------------------------------------
int ksolve_strided_launch(const LineGeom& g, const BandLU& f, const double* in, double* out, hipStream_t st);
int ksolve_rows_launch(const RowLines& g, const BandLU& f, const double* in, double* out, hipStream_t st);
int band_lu(int64_t n, int kl, int ku, double* ab, int64_t ldab, int* ipiv);
void band_lu_tables(int64_t n, int kl, int ku, const double* ab, int64_t ldab, const int* ipiv,
                    std::vector<double>& L, std::vector<double>& U, std::vector<int>& piv);

}  // namespace poms
