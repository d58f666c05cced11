// extern "C" boundary of libpoms_hip.so (declared in include/poms_hip.h): the error
// message, the context, and what runs per operator launch -- the setters, variant
// selection, launch geometry, partials placement, op_run with its wrappers and reductions,
// the split call and launch timing.  abi_op_setup.hip makes and destroys the operators.
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

// The values poms_op_set_variant accepts (include/poms_hip.h) and the fused epilogues each
// runs.  90/91, 92-100, 101-113: diagnostic / tuning builds of v3, v4, v5 (110-112: v5 two
// sweeps from zero without sums / x1 scaling, timing only; 113: the Jacobi sweep streaming
// the x rows no other tile reads) (11, v7, was removed in round 6: slower than v5)
enum : int { CAP_KNOWN = 1, CAP_APPLY_DOT = 2, CAP_FUSED_DOT = 4, CAP_FROM_ZERO = 8 };
static int variant_caps(int v) {
    switch (v) {
        case 0: return CAP_KNOWN;
        case 4: return CAP_KNOWN | CAP_APPLY_DOT | CAP_FUSED_DOT;
        case 7: return CAP_KNOWN | CAP_FUSED_DOT;
        case 8: case 9: case 10: return CAP_KNOWN | CAP_APPLY_DOT | CAP_FUSED_DOT | CAP_FROM_ZERO;
        case 110: case 111: case 112: return CAP_KNOWN | CAP_FROM_ZERO;
        case 114: return CAP_KNOWN | CAP_FUSED_DOT | CAP_FROM_ZERO;
    }
    return (v >= 90 && v <= 113) ? CAP_KNOWN : 0;
}
static bool variant_can(const poms_op* o, int cap) { return (variant_caps(o->variant) & cap) != 0; }

// rounds of `slots` resident workgroups for nc chunks of `tiles` tiles, a partial last round at 5x its fill
static double rounds(int nc, int tiles, double slots) {
    const double r = (double)nc * tiles / slots;
    const double fr = std::floor(r);
    return r > 1.0 ? fr + std::min(1.0, (r - fr) * 5.0) : 1.0;
}

// Axis-0 chunk length.  A workgroup streams `chunk` planes plus 2p halo planes, so
// long chunks save re-reads but leave a ragged last round of workgroups on the
// 256 CUs (512 resident workgroups at p <= 3).  Cost of nc chunks ~ rounds(nc) *
// (chunk + 2p) (fit to the chunk sweeps in profiles/r01/chunks/*.log; picks 103 at
// 515^3 p=3, 43 at 258^3 p=2).  For p >= 4 the kernels are VALU-bound and want >= 3
// workgroups per CU instead.
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
        const double cost = rounds(nc, tiles, slots) * (ch + 2 * p);
        if (cost < best - 1e-9) { best = cost; best_chunk = ch; }
    }
    return best_chunk;
}

// v5 (variant 10) runs 3D FORM_SUM operators, p <= 5, pads == pmax, arrays < 2 GiB.
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

// The launch geometry of kernel variant v (v5_to: v5's output columns per tile) for the
// request's planes.
static int op_geom(poms_op* o, const OpLaunch& q, KronGeom& g, int v, int v5_to) {
    const int epi = q.epi;
    const int64_t zb = q.zb, ze = q.ze, zb2 = q.zb2, ze2 = q.ze2;
    const bool is3d = o->ndim == 3;
    const RowGeom r = row_geom(&o->L);
    g.s0 = r.s0;
    g.s1 = r.s1;
    g.n0 = r.n0; g.n1 = r.n1; g.n2 = r.n2;
    g.pd0 = r.pd0; g.pd1 = r.pd1; g.pd2 = r.pd2;
    g.g0 = (int)o->g0;
    g.tiles2 = (int)((o->L.n[2] + kron_tile_cols() - 1) / kron_tile_cols());
    const int trows = v == 10 ? kron_v5_rows(o->pmax, epi, same_toeplitz12(o->tc, o->pmax) ? 1 : 0)
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
            one = nz + 2 * o->pmax <= 1.4 * rounds((nz + chunk - 1) / chunk, tiles, slots) * (chunk + 2 * o->pmax);
            if (one) chunk = nz;
        }
        // the v5 two-sweeps-from-zero launch (VALU-bound) balances better over twice
        // as many chunks: 515^3 p = 3, 86 instead of 172 planes, 836-838 against
        // 865-882 us in two interleaved sweeps, equal medians (833 us) in a third
        // (profiles/r03/chunks/); the other epilogues keep the model's pick (Jacobi
        // 715 us at 172 against 729 at 86)
        if (!one && v == 10 && epi == EPI_JACOBI0 && o->pmax == 3 && same_toeplitz12(o->tc, o->pmax) && chunk / 2 >= 8 * o->pmax)
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
    return general_form(o) || variant_can(o, CAP_FUSED_DOT);
}

// General-stencil launch (FORM_STENCIL): the epilogues of op_run plus EPI_DIAG.
static int stencil_run(poms_op* o, const OpLaunch& q) {
    const int epi = q.epi;
    const int64_t zb = q.zb, ze = q.ze, zb2 = q.zb2, ze2 = q.ze2;
    const bool want_norm = q.want_norm, want_dot = q.want_dot;
    if (q.route) q.route->used = false;   // (its own partials layout: the scratch only)
    if (epi == EPI_JACOBI0) { set_error("general stencil: no two-sweeps-from-zero epilogue"); return 1; }
    if (want_dot && epi != EPI_JACOBI && epi != EPI_APPLYDOT) { set_error("general stencil: dot needs Jacobi / apply+dot"); return 1; }
    const RowGeom r = row_geom(&o->L);
    if (zb < 0 || ze > r.n0 || zb > ze || zb2 < 0 || ze2 > r.n0 || zb2 > ze2) { set_error("general stencil: bad plane range"); return 1; }
    const StencilGeom g = stencil_geom(r, o->sp, zb, ze, zb2, ze2, o->dmask);
    const int maxb = (int)(kScratch / 2);
    int nb = 0;
    double* scr = o->ctx->scratch;
    const bool red = want_norm || want_dot || epi == EPI_APPLYDOT;
    if (stencil_launch(epi, g, o->coef, q.x, q.y, q.b, q.omega, want_norm ? scr : nullptr,
                       (want_dot || epi == EPI_APPLYDOT) ? scr + std::min<int64_t>(maxb, std::max<int64_t>(1, ((int64_t)(ze - zb + ze2 - zb2) * r.n1 * r.n2 + 255) / 256)) : nullptr,
                       maxb, as_stream(q.stream), &nb, q.beta))
        return 1;
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = red ? nb : 0;
    return 0;
}

// Matrix-free launch (FORM_MATFREE): stencil_run's epilogues and partials layout
// (norms at scratch[0, nb), dots behind them).  The whole grid in one launch: the
// operator is undistributed, so the plane range must be all of axis 0.  Nothing is
// allocated or synchronised here.
static int matfree_run(poms_op* o, const OpLaunch& q) {
    const int epi = q.epi;
    const bool want_norm = q.want_norm, want_dot = q.want_dot;
    if (q.route) q.route->used = false;   // (stencil_run's layout: the scratch only)
    if (epi == EPI_JACOBI0) { set_error("matrix-free operator: no two-sweeps-from-zero epilogue"); return 1; }
    if (want_dot && epi != EPI_JACOBI && epi != EPI_APPLYDOT) { set_error("matrix-free operator: dot needs Jacobi / apply+dot"); return 1; }
    const RowGeom r = row_geom(&o->L);
    if (q.zb != 0 || q.ze != r.n0 || q.zb2 != q.ze2) { set_error("matrix-free operator: the plane range must be the whole axis 0"); return 1; }
    const int maxb = (int)(kScratch / 2);
    double* scr = o->ctx->scratch;
    int nb = 0;
    if (epi == EPI_DIAG) {   // x = scale b / diag: the general stencil's kernel on the stored diagonal
        static const int point[3] = {0, 0, 0};   // (half-widths 0: one coefficient per row, and no mask)
        const StencilGeom g = stencil_geom(r, point, 0, r.n0, 0, 0, 0);
        if (stencil_launch(EPI_DIAG, g, o->mf_diag, q.x, q.y, q.b, q.omega, want_norm ? scr : nullptr, nullptr, maxb,
                           as_stream(q.stream), &nb))
            return 1;
        POMS_HIP_CHECK(hipGetLastError());
        o->last_partials = want_norm ? nb : 0;
        return 0;
    }
    if ((epi == EPI_JACOBI || epi == EPI_APPLYDOT || epi == EPI_CHEBY) && q.x == q.y) { set_error("matrix-free operator: y must not alias x"); return 1; }
    const MatfreeGeom& g = o->mf_geom;
    const int nblk = (int)std::min<int64_t>(g.ntiles, maxb);
    const bool wd = want_dot || epi == EPI_APPLYDOT;
    if (matfree_launch(epi, g, o->mf_ax, q.x, q.y, q.b, o->mf_a, o->mf_c, o->mf_diag, o->mf_mass, q.omega,
                       want_norm ? scr : nullptr, wd ? scr + nblk : nullptr, maxb, as_stream(q.stream), &nb,
                       o->mf_tensor, q.beta, &o->mf_faces))
        return 1;
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = (want_norm || wd) ? nb : 0;
    return 0;
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

// EPI_PAPPLYDOT (kron_v5.hip): y2 = b + beta x formed inside the apply + dot of y2.  It runs
// where v5 runs its 16-wave tiles (3D FORM_SUM, p <= 3; not the diagnostic builds) on one
// rank without ghost data (the launch stores y2's interior points only: its pads must be
// zero already, as the flat update would have written them), and where the launch takes the
// tile geometry of the apply + dot on y2 it replaces, so that q and the p.q partials keep
// their bits: x and y2 on the same side of v5's line alignment.
bool poms::papply_ok(const poms_op* o, const double* x, const double* b, const double* y2, const double* y) {
    if (!o || !x || !b || !y2 || !y || x == b || x == y2 || x == y || b == y2 || b == y || y2 == y) return false;
    if (general_form(o) || distributed(o) || o->pmax > 3 || o->variant > 10) return false;
    if (resolve_variant(o, EPI_PAPPLYDOT) != 10) return false;
    return v5_aligned(o, x) == v5_aligned(o, y2);
}

// EPI_RJACOBI0 (kron_v5_kernel.hpp): y2 = x - alpha b formed inside the two sweeps from zero
// on y2.  It runs where those sweeps run the 16-wave v5 build (3D FORM_SUM, p = 3, axes 1 and
// 2 sharing their Toeplitz rows; not the diagnostic builds) on one rank without ghost data
// (the launch stores y2's interior points only: its pads must be zero already), and where the
// launch takes the tile geometry of the sweeps on y2 it replaces, so that their sums keep
// their bits: x, b and y2 on the same side of v5's line alignment.
bool poms::rfold_ok(const poms_op* o, const double* x, const double* b, const double* y2, const double* y) {
    if (!o || !x || !b || !y2 || !y || x == b || x == y2 || x == y || b == y2 || b == y || y2 == y) return false;
    if (general_form(o) || distributed(o) || o->ndim != 3 || o->pmax != 3 || o->variant > 10) return false;
    if (!variant_can(o, CAP_FROM_ZERO) || resolve_variant(o, EPI_JACOBI0) != 10) return false;
    if (!same_toeplitz12(o->tc, o->pmax) || padded_len(o) * 8 >= 0x7ffffff0LL) return false;
    return v5_aligned(o, x) == v5_aligned(o, y2) && v5_aligned(o, x) == v5_aligned(o, b);
}

// Two Jacobi sweeps per launch (EPI_JACOBI2, kron_2d.hip): one-rank 2D p = 3
// Kronecker operators whose single sweep runs the v3 whole-array kernel (variant 9),
// whose bits the two-sweep kernel reproduces
bool poms::sweep2_ok(const poms_op* o) {
    if (o->ndim != 2 || o->pmax != 3 || general_form(o) || o->ghost_corners) return false;
    if (o->L.pads[1] != 3 || o->L.pads[2] != 3 || resolve_variant(o, EPI_JACOBI) != 9) return false;
    return padded_len(o) * 8 < 0x7ffffff0LL;
}

// Where a launch of nblk blocks writes its partials (none wanted: null pointers): the
// route's destination when its sums fit there (route->used), norms at *pn and dots behind
// them at *pd; else the scratch, norms at part_off and dots at dot_base (default nblk) +
// part_off.  The scratch must hold them even when the route takes them.  `three`
// (EPI_JACOBI3Z): three sums side by side from *pn, which the scratch holds only in its
// default layout and need not hold when the route takes them.
// `extra` (EPI_RJACOBI0: 1): further sums of nblk partials behind the dots, in the scratch's
// default layout only.
static int part_place(poms_op* o, int64_t nblk, bool wn, bool wd, bool three, PartRoute* route, double** pn,
                      double** pd, int extra = 0) {
    if (route) route->used = false;
    *pn = *pd = nullptr;
    if (!wn && !wd) return 0;
    const int64_t dbase = o->dot_base < 0 ? nblk : o->dot_base;
    const bool fits = three ? o->part_off == 0 && o->dot_base < 0 && 3 * nblk <= kScratch
                    : extra ? o->part_off == 0 && o->dot_base < 0 && (2 + extra) * nblk <= kScratch
                            : o->part_off + nblk <= dbase && dbase + o->part_off + nblk <= kScratch;
    const bool sink = route && route->dst && (three ? 3 : (wn ? 1 : 0) + (wd ? 1 : 0) + extra) * nblk <= route->cap;
    if (!fits && !(three && sink)) { set_error("too many blocks for the partial-sum scratch"); return 1; }
    *pn = sink ? route->dst : o->ctx->scratch + o->part_off;
    *pd = sink ? route->dst + (wn ? nblk : 0) : o->ctx->scratch + dbase + o->part_off;
    if (sink) route->used = true;
    return 0;
}

// partials as op_run: norm (sweep k+1) and dot (sweep k) at the route's destination / the
// scratch.  EPI_JACOBI3Z (x = b): all three sums or none, ||x1||^2, ||dr_2||^2, ||dr_3||^2
// side by side (the route's destination, or scratch[0, 3n))
static int op_run_j2(poms_op* o, const OpLaunch& q) {
    const double *x = q.x, *b = q.b;
    double* y = q.y;
    const bool want_norm = q.want_norm, want_dot = q.want_dot;
    if (!sweep2_ok(o)) { set_error("two sweeps per launch: one-rank 2D p = 3 Kronecker operators (variant 9) only"); return 1; }
    if (x == y || b == y) { set_error("two sweeps per launch: x_out must not alias x_in or b"); return 1; }
    const bool fz = q.epi == EPI_JACOBI3Z;
    if (fz && (x != b || want_norm != want_dot)) { set_error("three sweeps from zero: x = b, all three sums or none"); return 1; }
    KronGeom g;
    if (op_geom(o, q, g, 9, 0)) return 1;   // (2D: the request's planes and epilogue do not enter)
    const int trows = fz ? kron2d_j2_rows_default() : kron2d_j2_rows();
    g.tout = kron2d_j2_cols(o->pmax);
    g.tiles2 = (int)((o->L.n[2] + g.tout - 1) / g.tout);
    g.tiles1 = (int)((o->L.n[1] + trows - 1) / trows);
    const int64_t nblk = (int64_t)g.tiles2 * g.tiles1;
    o->last_variant = 9;
    if (nblk == 0) { o->last_partials = 0; return 0; }
    double *pn = nullptr, *pd = nullptr;
    if (part_place(o, nblk, want_norm, want_dot, fz, q.route, &pn, &pd)) return 1;
    if (fz) {   // (pn: the three sums' base, pd = pn + nblk)
        KronPtrs p{b, y, b, o->a0t, o->b0t, o->a1, o->b1, o->a2, o->b2, pn ? pn + 2 * nblk : nullptr, pd, nullptr};
        if (kron2d_j2_launch(o->pmax, o->form, p, g, o->tc, q.omega, as_stream(q.stream), true, pn)) return 1;
        POMS_HIP_CHECK(hipGetLastError());
        o->last_partials = want_norm ? nblk : 0;
        return 0;
    }
    KronPtrs p{x, y, b, o->a0t, o->b0t, o->a1, o->b1, o->a2, o->b2, want_norm ? pn : nullptr,
               want_dot ? pd : nullptr, nullptr};
    if (kron2d_j2_launch(o->pmax, o->form, p, g, o->tc, q.omega, as_stream(q.stream), false, nullptr)) return 1;
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = (want_norm || want_dot) ? nblk : 0;
    return 0;
}

// Launch timing around op_run's launch: *tl is the event pair of a sampled launch (null: not
// timed), *ext whether its events ride on the v5 dispatch.
static int timing_begin(poms_op* o, const OpLaunch& q, int v, const KronGeom& g, poms_op::TimedLaunch** tl, bool* ext) {
    poms_op::TimedLaunch*& tlh = *tl;
    if (o->timing && (o->t_epi < 0 || o->t_epi == q.epi) && (o->t_seen++ % o->t_every) == 0) {
        // events on the launch stream around this launch (a sample: every t_every-th)
        if (o->tl_used == o->tl.size()) {
            poms_op::TimedLaunch ev{};
            POMS_HIP_CHECK(hipEventCreate(&ev.e0));
            POMS_HIP_CHECK(hipEventCreate(&ev.e1));
            o->tl.push_back(ev);
        }
        tlh = &o->tl[o->tl_used++];
        tlh->epi = q.epi;
        tlh->ndof = (int64_t)((q.ze - q.zb) + (q.ze2 - q.zb2)) * g.n1 * g.n2;
        // v5 outside a capture: the events ride on the kernel's own dispatch
        // (hipExtLaunchKernel start / stop), i.e. the kernel's execution time as
        // rocprofv3 reports it; otherwise event records before and after the launch
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        POMS_HIP_CHECK(hipStreamIsCapturing(as_stream(q.stream), &cs));
        if (v == 10 && cs == hipStreamCaptureStatusNone) {
            kron_v5_set_launch_events(tlh->e0, tlh->e1);
            *ext = true;
        } else {
            POMS_HIP_CHECK(timing_record(tlh->e0, as_stream(q.stream)));
        }
    }
    return 0;
}

static int timing_end(const OpLaunch& q, poms_op::TimedLaunch* tlh, bool tl_ext, int rc) {   // (rc: the launch's)
    if (tl_ext && !kron_v5_launch_events_used()) {   // (the v5 launch failed before its dispatch)
        kron_v5_set_launch_events(nullptr, nullptr);
        if (!rc) { set_error("v5: timed launch did not take its events"); return 1; }
    }
    if (tlh && !tl_ext) POMS_HIP_CHECK(timing_record(tlh->e1, as_stream(q.stream)));
    return 0;
}

// One launch: resolve the variant, its geometry, place the partials, launch.
static int op_run(poms_op* o, const OpLaunch& q) {
    const int epi = q.epi;
    const bool want_norm = q.want_norm, want_dot = q.want_dot;
    if (!o || !q.x || !q.y) { set_error("null operator or vector"); return 1; }
    if (epi != EPI_APPLY && !q.b) { set_error("null right-hand side"); return 1; }
    if (epi == EPI_PAPPLYDOT && (!q.beta_dev || !papply_ok(o, q.x, q.b, q.y2, q.y))) {
        set_error("p update + apply + x.y: v5's 16-wave tiles on one rank, five distinct arguments (poms_op_papply_dot_supported)");
        return 1;
    }
    if (epi == EPI_RJACOBI0 && (!q.beta_dev || !rfold_ok(o, q.x, q.b, q.y2, q.y))) {
        set_error("r update + two sweeps from zero: v5's p = 3 16-wave tiles on one rank, four distinct arguments (poms_op_rjacobi0_supported)");
        return 1;
    }
    if (epi == EPI_JACOBI2 || epi == EPI_JACOBI3Z) return op_run_j2(o, q);
    if (o->form == FORM_STENCIL) return stencil_run(o, q);
    if (o->form == FORM_MATFREE) return matfree_run(o, q);
    if (epi == EPI_CHEBY) { set_error("Chebyshev step: general-stencil and matrix-free operators only"); return 1; }
    if (epi == EPI_APPLYDOT && !variant_can(o, CAP_APPLY_DOT)) {
        set_error("apply + x.y: kernel variants 4, 8, 9, 10 only");
        return 1;
    }
    if (want_dot && ((epi != EPI_JACOBI && epi != EPI_JACOBI0 && epi != EPI_APPLYDOT && epi != EPI_PAPPLYDOT &&
                      epi != EPI_RJACOBI0) ||
                     !fused_dot_ok(o))) {
        set_error("fused x_out.b needs a Jacobi sweep on kernel variants 4-10");
        return 1;
    }
    if (epi == EPI_JACOBI0 && !variant_can(o, CAP_FROM_ZERO)) {
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
    // (EPI_RJACOBI0: the variant, tiles and chunks of the two sweeps from zero it contains)
    const int gepi = epi == EPI_RJACOBI0 ? (int)EPI_JACOBI0 : epi;
    int v = resolve_variant(o, gepi);
    const int v5_diag = (v >= 101 && v <= 114) ? v - 100 : 0;   // v5 diagnostic / tuning builds
    if (v5_diag) v = 10;
    o->last_variant = v5_diag ? 100 + v5_diag : v;
    int v5_h = 0, v5_to = 0;
    if (v == 10) kron_v5_tile(o->pmax, v5_aligned(o, q.x), &v5_h, &v5_to);
    KronGeom g;
    OpLaunch qg = q;
    qg.epi = gepi;
    if (op_geom(o, qg, g, v, v5_to)) return 1;
    const int64_t nblk = (int64_t)g.tiles2 * g.tiles1 * g.nchunks;
    if (nblk == 0) { o->last_partials = 0; return 0; }
    double *pn = nullptr, *pd = nullptr;
    // (EPI_RJACOBI0's third sum, ||y2||^2: nblk partials behind the dots)
    if (part_place(o, nblk, want_norm, want_dot, false, q.route, &pn, &pd, epi == EPI_RJACOBI0 && want_dot ? 1 : 0))
        return 1;
    KronPtrs p{q.x, q.y, q.b, o->a0t, o->b0t, o->a1, o->b1, o->a2, o->b2, want_norm ? pn : nullptr,
               want_dot ? pd : nullptr, o->rdiag0, q.y2, q.beta_dev};
    poms_op::TimedLaunch* tlh = nullptr;
    bool tl_ext = false;
    if (timing_begin(o, q, v, g, &tlh, &tl_ext)) return 1;
    const hipStream_t st = as_stream(q.stream);
    const int rc = v == 10
        ? kron_v5_launch(o->pmax, epi, p, g, o->tc, v5_h, q.omega, st, v5_diag)
        : v == 0
        ? kron_launch(o->pmax, o->ndim == 3, o->form, epi, p, g, q.omega, st)
        : (v == 7 || (v >= 92 && v <= 100))
        ? kron_v4_launch(o->pmax, o->ndim == 3, o->form, epi, p, g, o->tc, q.omega, st, v == 7 ? 0 : v - 91)
        : kron_v3_launch(v, o->pmax, o->ndim == 3, o->form, epi, p, g, o->tc, q.omega, st);
    if (timing_end(q, tlh, tl_ext, rc) || rc) return 1;
    POMS_HIP_CHECK(hipGetLastError());
    o->last_partials = (want_norm || want_dot) ? nblk : 0;
    if (epi == EPI_PAPPLYDOT) ++o->papply_launches;
    if (epi == EPI_RJACOBI0) ++o->rfold_launches;
    return 0;
}

// the forms and layouts whose Chebyshev step is one launch: the general forms, undistributed
static bool cheby_ok(const poms_op* o) {
    return general_form(o) && !distributed(o);
}

// One launch of the request, its partials written to the route's destination where one
// is given and they fit, else where op->part_off / dot_base say (part_place); the argument
// checks of poms_op_run_reduce2, then the fields an epilogue fixes, then the launch.
int poms::op_run_epi(poms_op* op, const OpLaunch& in) {
    OpLaunch q = in;
    const bool wn = q.want_norm, wd = q.want_dot;
    const bool planes_2d = q.zb == 0 && q.ze == 1 && q.zb2 == q.ze2;
    int fz = 0;
    switch (q.epi) {
        case EPI_APPLY:
            if (wn || wd) { set_error("poms_op_run_reduce: apply has no reductions"); return 1; }
            break;
        case EPI_RESID:
            if (wn || wd) { set_error("poms_op_run_reduce: residual has no reductions"); return 1; }
            break;
        case EPI_JACOBI:
            if (q.x == q.y) { set_error("jacobi sweep: x_out must not alias x_in"); return 1; }
            break;
        case EPI_JACOBI0:   // x = b: norm_out <- ||dr_2||^2, dot_out <- ||x1||^2
            if (poms_op_from_zero_supported(op, &fz)) return 1;
            if (!fz) { set_error("jacobi from zero: not supported by this operator"); return 1; }
            if (q.b == q.y) { set_error("jacobi from zero: x_out must not alias b"); return 1; }
            if (wn != wd) { set_error("jacobi from zero: both norms or neither"); return 1; }
            break;
        case EPI_JACOBI2:   // two sweeps from x: norm_out <- ||dr_{k+1}||^2, dot_out <- ||dr_k||^2
            if (!planes_2d) { set_error("two sweeps per launch: 2D (planes [0, 1))"); return 1; }
            break;
        case EPI_JACOBI3Z:   // sweeps 1-3 from x = 0 (x = b): norm_out <- ||dr_3||^2, dot_out <- ||dr_2||^2
            // (poms_op_run_reduce2 cannot return the third sum: poms_op_jacobi3_from_zero)
            if (!planes_2d) { set_error("three sweeps from zero: 2D (planes [0, 1))"); return 1; }
            break;
        case EPI_APPLYDOT:
            if (q.x == q.y) { set_error("apply: y must not alias x"); return 1; }
            if (wn || !wd) { set_error("apply + dot: dot_out only"); return 1; }
            break;
        case EPI_RJACOBI0:   // y2 = x - alpha b, two sweeps from zero on y2: the sums of EPI_JACOBI0, and ||y2||^2
            // (poms_op_run_reduce cannot name y2 and alpha: not one of its epilogues)
            if (!q.y2 || !q.beta_dev) { set_error("poms_op_run_reduce: bad epilogue"); return 1; }
            if (wn != wd) { set_error("r update + jacobi from zero: all three sums or none"); return 1; }
            break;
        case EPI_PAPPLYDOT:   // y2 = b + beta x, y = A y2, dot_out <- y2 . y
            // (poms_op_run_reduce cannot name y2 and beta: not one of its epilogues)
            if (!q.y2 || !q.beta_dev) { set_error("poms_op_run_reduce: bad epilogue"); return 1; }
            if (wn || !wd) { set_error("p update + apply + dot: dot_out only"); return 1; }
            break;
        default:
            set_error("poms_op_run_reduce: bad epilogue");
            return 1;
    }
    // what an epilogue fixes (the 2D ones' planes are [0, 1) already)
    const int e = q.epi;
    if (e == EPI_APPLY) q.b = nullptr;
    if (e == EPI_APPLYDOT) q.b = q.x;
    if (e == EPI_APPLY || e == EPI_RESID || e == EPI_APPLYDOT || e == EPI_PAPPLYDOT) q.omega = 0.0;
    if (e == EPI_APPLY || e == EPI_RESID) q.route = nullptr;   // (no sums: the route stays as it came)
    if (e == EPI_JACOBI0 || e == EPI_JACOBI3Z) q.x = q.b;
    if (e == EPI_JACOBI2 || e == EPI_JACOBI3Z) q.zb2 = q.ze2 = 0;
    return op_run(op, q);
}

namespace poms {
// The distributed operator call's two launches -- the request `in` (its planes [zb, ze)
// only, the sums the two outputs ask for) on its stream, then the same over
// the boundary ranges [b1s, b1e) + [b2s, b2e) once the ghost exchange is done --
// with both launches' partials side by side in the scratch and ONE reduction per
// requested sum after both (one launch fewer per sum than reducing each launch;
// poms_op_run_dist).  The boundary launch goes to h.bstream when given (the
// communication stream, right behind the exchange): it depends on the exchange
// only, not on the interior launch, so its workgroups fill the CUs the interior
// launch's last round leaves idle instead of running as a separate, mostly empty
// round of its own; `stream` then waits for it (h.join) before the reductions.
int op_run_split(poms_op* op, const OpLaunch& in, int64_t b1s, int64_t b1e, int64_t b2s, int64_t b2e,
                 double* norm_out, double* dot_out, const SplitHooks& h) {
    if (!op) { set_error("op_run_split: null operator"); return 1; }
    void* const stream = in.stream;
    if (general_form(op)) {   // its own partials layout: reduce each launch, both on `stream`
        if (poms_op_run_reduce2(op, in.epi, in.omega, in.x, in.y, in.b, in.zb, in.ze, 0, 0, norm_out, dot_out, 0, stream))
            return 1;
        if (h.ghosts_on(h.arg, stream)) return 1;
        return poms_op_run_reduce2(op, in.epi, in.omega, in.x, in.y, in.b, b1s, b1e, b2s, b2e, norm_out, dot_out, 1, stream);
    }
    const bool wn = norm_out != nullptr, wd = dot_out != nullptr;
    OpLaunch q{in.epi, in.x, in.y, in.b, in.zb, in.ze, stream, in.omega, wn, wd};   // the interior, then the boundaries
    struct Reset {
        poms_op* o;
        ~Reset() { o->part_off = 0; o->dot_base = -1; }
    } reset{op};
    op->part_off = 0;
    op->dot_base = kScratch / 2;
    op->split_interior = true;
    const int rci = op_run_epi(op, q);
    op->split_interior = false;
    if (rci) return 1;
    const int64_t n1 = op->last_partials;
    void* bs = h.bstream ? h.bstream : stream;
    if (h.ghosts_on(h.arg, bs)) return 1;
    op->part_off = n1;
    q.zb = b1s; q.ze = b1e; q.zb2 = b2s; q.ze2 = b2e;
    q.stream = bs;
    if (op_run_epi(op, q)) return 1;
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

int poms_op_set_variant(poms_op* op, int variant) {
    if (!op || !(variant_caps(variant) & CAP_KNOWN)) {
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

int poms_variant_built(int variant) { return (variant_caps(variant) & CAP_KNOWN) ? 1 : 0; }

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

// A stream capture is in progress, as far as a call without a stream argument can see one:
// the legacy stream answers for a capture on any stream of the thread in the global capture
// mode; the operator's own capture stream is asked as well.
static bool capture_in_progress(const poms_op* op) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    bool capturing = hipStreamIsCapturing(nullptr, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    if (!capturing && op->cap_stream)
        capturing = hipStreamIsCapturing(op->cap_stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    if (capturing) (void)hipGetLastError();
    return capturing;
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
    if (distributed(op)) {
        set_error(fn + "distributed operators (slabs, Cart blocks) are not supported");
        return 1;
    }
    if (capture_in_progress(op)) { set_error(fn + "called during a stream capture"); return 1; }
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

// A face term of a general form (the face mass of a Robin condition): see the header.  A
// set-up call: every check comes first, the launch runs on the null stream and the call ends
// in a device synchronise.
int poms_op_add_face_term(poms_op* op, int axis, int side, const double* coef_host, const int64_t* m,
                          const int* half) {
    const std::string fn = "poms_op_add_face_term: ";
    if (!op || !coef_host || !m || !half) { set_error(fn + "null argument"); return 1; }
    if (!general_form(op)) {
        set_error(fn + "Kronecker forms take a Robin term through their factors (needs a general-stencil or matrix-free operator)");
        return 1;
    }
    if (axis < 0 || axis >= op->ndim) { set_error(fn + "axis must be 0 .. ndim - 1 = " + std::to_string(op->ndim - 1)); return 1; }
    if (side != 0 && side != 1) { set_error(fn + "side must be 0 or 1"); return 1; }
    if (distributed(op)) {
        set_error(fn + "distributed operators (slabs, Cart blocks) are not supported");
        return 1;
    }
    const RowGeom r = row_geom(&op->L);
    const int ax = axis + (3 - op->ndim);   // the operator's axes are the kernels' last ndim
    const int a = ax == 0 ? 1 : 0, b = ax == 2 ? 1 : 2;
    const int n[3] = {r.n0, r.n1, r.n2};
    if (m[0] != n[a] || m[1] != n[b] || half[0] != op->sp[a] || half[1] != op->sp[b]) {
        set_error(fn + "m and half must be the operator's extents and half-widths on the face's axes: (" +
                  std::to_string(n[a]) + ", " + std::to_string(n[b]) + ") and (" + std::to_string(op->sp[a]) + ", " +
                  std::to_string(op->sp[b]) + ")");
        return 1;
    }
    if (capture_in_progress(op)) { set_error(fn + "called during a stream capture"); return 1; }
    POMS_HIP_CHECK(hipSetDevice(op->ctx->device));
    const int f = 2 * ax + side;
    const size_t len = (size_t)n[a] * n[b] * (2 * op->sp[a] + 1) * (2 * op->sp[b] + 1);
    const StencilGeom g = stencil_geom(r, op->sp, 0, r.n0, 0, 0, 0);
    double* d = nullptr;
    if (upload(coef_host, len, &d)) return 1;
    // a matrix-free face keeps the sum of every call's stencil, on the host and on the device:
    // a later call re-uploads the sum first, so that a failed copy leaves the diagonal untouched
    const bool again = op->form == FORM_MATFREE && !op->mf_face_host[f].empty();
    std::vector<double> sum;
    if (again) {
        sum = op->mf_face_host[f];
        for (size_t k = 0; k < len; ++k) sum[k] += coef_host[k];
        if (hipMemcpy(const_cast<double*>(op->mf_faces.s[f]), sum.data(), len * sizeof(double),
                      hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(d);
            set_error(fn + "the copy of the face stencil failed");
            return 1;
        }
    }
    face_add_launch(g, ax, side, d, op->form == FORM_STENCIL ? op->coef : nullptr,
                    op->form == FORM_MATFREE ? op->mf_diag : nullptr, nullptr);
    const bool ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (ok && op->form == FORM_MATFREE) {
        if (again) {
            op->mf_face_host[f].swap(sum);
        } else {
            op->mf_face_host[f].assign(coef_host, coef_host + len);
            op->mf_faces.s[f] = d;   // (the handle owns it from here)
            d = nullptr;
        }
        op->mf_faces.mask |= 1 << f;
    }
    if (d) (void)hipFree(d);
    if (!ok) { set_error(fn + "the launch failed"); return 1; }
    op->fmask |= 1 << f;
    ++op->gen;
    return 0;
}

int poms_op_face_terms(poms_op* op, int* faces) {
    if (!op || !faces) { set_error("poms_op_face_terms: null argument"); return 1; }
    *faces = op->fmask >> (2 * (3 - op->ndim));
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

int poms_op_apply(poms_op* op, const double* x, double* y, int64_t zb, int64_t ze, void* stream) {
    return op_run(op, OpLaunch{EPI_APPLY, x, y, nullptr, zb, ze, stream});
}

int poms_op_residual(poms_op* op, const double* b, const double* x, double* r, int64_t zb,
                     int64_t ze, void* stream) {
    return op_run(op, OpLaunch{EPI_RESID, x, r, b, zb, ze, stream});
}

int poms_op_jacobi_sweep(poms_op* op, double omega, const double* b, const double* x_in,
                         double* x_out, int64_t zb, int64_t ze, int want_norm, void* stream) {
    if (x_in == x_out) { set_error("jacobi sweep: x_out must not alias x_in"); return 1; }
    return op_run(op, OpLaunch{EPI_JACOBI, x_in, x_out, b, zb, ze, stream, omega, want_norm != 0});
}

int poms_op_jacobi_sweep_dot(poms_op* op, double omega, const double* b, const double* x_in,
                             double* x_out, int64_t zb, int64_t ze, int want_norm, void* stream) {
    if (x_in == x_out) { set_error("jacobi sweep: x_out must not alias x_in"); return 1; }
    return op_run(op, OpLaunch{EPI_JACOBI, x_in, x_out, b, zb, ze, stream, omega, want_norm != 0, true});
}

int poms_op_apply_dot(poms_op* op, const double* x, double* y, int64_t zb, int64_t ze, void* stream) {
    if (x == y) { set_error("apply: y must not alias x"); return 1; }
    return op_run(op, OpLaunch{EPI_APPLYDOT, x, y, x, zb, ze, stream, 0.0, false, true});
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
    OpLaunch q{EPI_CHEBY, x, y, b, zb, ze, stream, alpha};
    q.beta = beta;
    return op_run(op, q);
}

int poms_op_cheby_supported(poms_op* op, int* yes) {
    if (!op || !yes) { set_error("poms_op_cheby_supported: null argument"); return 1; }
    *yes = cheby_ok(op) ? 1 : 0;
    return 0;
}

int poms_op_apply_dot_supported(poms_op* op, int* yes) {
    if (!op || !yes) { set_error("poms_op_apply_dot_supported: null argument"); return 1; }
    *yes = (general_form(op) || variant_can(op, CAP_APPLY_DOT)) ? 1 : 0;
    return 0;
}

int poms_op_papply_dot_supported(poms_op* op, const double* s, const double* p, const double* p_next, const double* q,
                                 int* yes) {
    if (!op || !yes) { set_error("poms_op_papply_dot_supported: null argument"); return 1; }
    *yes = papply_ok(op, p, s, p_next, q) ? 1 : 0;
    return 0;
}

int poms_op_papply_dot(poms_op* op, const double* beta_dev, const double* s, const double* p, double* p_next,
                       double* q, double* dot_out, void* stream) {
    if (!op || !beta_dev || !s || !p || !p_next || !q || !dot_out) { set_error("poms_op_papply_dot: null argument"); return 1; }
    OpLaunch l{EPI_PAPPLYDOT, p, q, s, 0, op->L.n[0], stream, 0.0, false, true};
    l.y2 = p_next;
    l.beta_dev = beta_dev;
    if (op_run_epi(op, l)) return 1;
    const int64_t n = op->last_partials;
    if (reduce_launch(op->ctx->scratch + n, (int)n, dot_out, as_stream(stream))) {
        set_error("poms_op_papply_dot: reduction launch failed");
        return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_op_papply_dot_count(poms_op* op, int64_t* count) {
    if (!op || !count) { set_error("poms_op_papply_dot_count: null argument"); return 1; }
    *count = op->papply_launches;
    return 0;
}

int poms_op_rjacobi0_supported(poms_op* op, const double* r, const double* q, const double* r_new, const double* x_out,
                               int* yes) {
    if (!op || !yes) { set_error("poms_op_rjacobi0_supported: null argument"); return 1; }
    *yes = rfold_ok(op, r, q, r_new, x_out) ? 1 : 0;
    return 0;
}

int poms_op_rjacobi0(poms_op* op, double omega, const double* alpha_dev, const double* r, const double* q,
                     double* r_new, double* x_out, double* sums_out, void* stream) {
    if (!op || !alpha_dev || !r || !q || !r_new || !x_out) { set_error("poms_op_rjacobi0: null argument"); return 1; }
    const bool ws = sums_out != nullptr;
    OpLaunch l{EPI_RJACOBI0, r, x_out, q, 0, op->L.n[0], stream, omega, ws, ws};
    l.y2 = r_new;
    l.beta_dev = alpha_dev;
    if (op_run_epi(op, l)) return 1;
    if (!ws) return 0;
    const int64_t n = op->last_partials;   // (||dr_2||^2, ||x1||^2, ||r_new||^2: n partials each)
    const double* scr = op->ctx->scratch;
    if (reduce_launch(scr, (int)n, sums_out, as_stream(stream)) ||
        reduce_launch(scr + n, (int)n, sums_out + 1, as_stream(stream)) ||
        reduce_launch(scr + 2 * n, (int)n, sums_out + 2, as_stream(stream))) {
        set_error("poms_op_rjacobi0: reduction launch failed");
        return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_op_rjacobi0_count(poms_op* op, int64_t* count, int64_t* exact) {
    if (!op || !count) { set_error("poms_op_rjacobi0_count: null argument"); return 1; }
    *count = op->rfold_launches;
    if (exact) *exact = op->rfold_exact;
    return 0;
}

int poms_op_jacobi_from_zero(poms_op* op, double omega, const double* b, double* x_out,
                             int64_t zb, int64_t ze, int want_norm, void* stream) {
    if (!op || !b || !x_out) { set_error("jacobi from zero: null argument"); return 1; }
    if (b == x_out) { set_error("jacobi from zero: x_out must not alias b"); return 1; }
    int yes = 0;
    if (poms_op_from_zero_supported(op, &yes)) return 1;
    if (!yes) { set_error("jacobi from zero: not supported by this operator (poms_op_from_zero_supported)"); return 1; }
    return op_run(op, OpLaunch{EPI_JACOBI0, b, x_out, b, zb, ze, stream, omega, want_norm != 0, want_norm != 0});
}

int poms_op_from_zero_supported(poms_op* op, int* yes) {
    if (!op || !yes) { set_error("poms_op_from_zero_supported: null argument"); return 1; }
    const int64_t bytes = padded_len(op) * 8;
    // 2D (round 6, v3): not on a block of a decomposition (its ghost rows' x1 would need
    // the neighbours' diagonal)
    *yes = ((op->ndim == 3 || (op->ndim == 2 && !op->ghost_corners)) && !general_form(op) &&
            variant_can(op, CAP_FROM_ZERO) && bytes < 0x7ffffff0LL) ? 1 : 0;
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
    if (op_run(op, OpLaunch{EPI_JACOBI3Z, b, x_out, b, 0, 1, stream, omega, wn, wn})) return 1;
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
    if (general_form(o)) {
        const OpLaunch q{EPI_DIAG, b, x, b, 0, o->L.n[0], stream, scale, want_norm != 0};
        return o->form == FORM_STENCIL ? stencil_run(o, q) : matfree_run(o, q);
    }
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
int poms_op_run_reduce2(poms_op* op, int epilogue, double omega, const double* x, double* y,
                        const double* b, int64_t zb, int64_t ze, int64_t zb2, int64_t ze2,
                        double* norm_out, double* dot_out, int accumulate, void* stream) {
    if (!op) { set_error("poms_op_run_reduce: null operator"); return 1; }
    const bool wn = norm_out != nullptr, wd = dot_out != nullptr;
    if (op_run_epi(op, OpLaunch{epilogue, x, y, b, zb, ze, stream, omega, wn, wd, nullptr, zb2, ze2})) return 1;
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

}  // extern "C"
