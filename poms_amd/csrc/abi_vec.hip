// extern "C" boundary of libpoms_hip.so (declared in include/poms_hip.h): the vector
// algebra on the padded layout, pcg's vector updates and the partial-sum reductions.
#include "common.hpp"
#include "launchers.hpp"
#include "split_hooks.hpp"
#include "abi_internal.hpp"
#include "../../include/poms_hip.h"

#include <cstdlib>

using namespace poms;

extern "C" {

// ---- vector kernels -----------------------------------------------------------
static int vec_common(poms_ctx* ctx, const poms_layout* L, int op, double a, double b,
                      const double* x, const double* y, double* z, double* w, const double* q,
                      double* out_dev, void* stream, const double* ab_dev = nullptr) {
    if (!ctx || !layout_ok(L)) { set_error("vector op: bad context or layout"); return 1; }
    const RowGeom g = row_geom(L);
    int nb = 0;
    const bool red = (op == V_DOT || op == V_PCGUPD || op == V_RUPD || op == V_FINUPD);
    // whole interior planes as one flat range (ghost rows / columns are zero in every
    // vector and stay zero -- unless the layout says they hold a neighbour's data);
    // the per-row kernel for fills, mixed alignments and ghost data
    const FlatRange fr = flat_range(g);
    auto at = [&](const double* v) { return v ? v + fr.off : nullptr; };
    const bool flat = !(L->flags & POMS_LAYOUT_GHOST_DATA) &&
                      vec_flat_launch(op, fr.count, a, b, at(x), at(y), const_cast<double*>(at(z)),
                                      const_cast<double*>(at(w)), at(q), red ? ctx->scratch : nullptr,
                                      as_stream(stream), &nb, ab_dev) == 0;
    if (!flat && vec_launch(op, g, a, b, x, y, z, w, q, red ? ctx->scratch : nullptr, as_stream(stream), &nb,
                            ab_dev))
        return 1;
    if (red) reduce_wide_launch(ctx->scratch, nb, out_dev, as_stream(stream));
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_vec_axpby(poms_ctx* ctx, const poms_layout* L, double a, const double* x, double b,
                   const double* y, double* z, void* stream) {
    if (!x || !y || !z) { set_error("axpby: null vector"); return 1; }
    return vec_common(ctx, L, V_AXPBY, a, b, x, y, z, nullptr, nullptr, nullptr, stream);
}

int poms_vec_scale(poms_ctx* ctx, const poms_layout* L, double a, const double* x, double* z,
                   void* stream) {
    if (!x || !z) { set_error("scale: null vector"); return 1; }
    return vec_common(ctx, L, V_SCALE, a, 0.0, x, nullptr, z, nullptr, nullptr, nullptr, stream);
}

}  // extern "C"

// z = x and z.z into out_dev in one pass (pcg from x0 = None: r = b, ||r||^2), with the
// bits of poms_vec_scale(1.0) + poms_vec_dot(z, z): the same flat grid, the same
// per-thread order.  Where the flat kernel does not apply (mixed alignment, ghost
// data) the two calls.
int poms::vec_copy_dot(poms_ctx* ctx, const poms_layout* L, const double* x, double* z, double* out_dev,
                       void* stream) {
    if (!ctx || !layout_ok(L) || !x || !z || !out_dev) { set_error("copy_dot: bad argument"); return 1; }
    const FlatRange fr = flat_range(row_geom(L));
    int nb = 0;
    static const bool cd_off = [] { const char* e = getenv("POMS_COPY_DOT"); return e && e[0] == '0'; }();
    if (!cd_off && !(L->flags & POMS_LAYOUT_GHOST_DATA) &&
        vec_flat_launch(V_SCALEDOT, fr.count, 1.0, 0.0, x + fr.off, nullptr, z + fr.off, nullptr, nullptr, ctx->scratch,
                        as_stream(stream), &nb) == 0) {
        reduce_wide_launch(ctx->scratch, nb, out_dev, as_stream(stream));
        POMS_HIP_CHECK(hipGetLastError());
        return 0;
    }
    return poms_vec_scale(ctx, L, 1.0, x, z, stream) || poms_vec_dot(ctx, L, z, z, out_dev, stream);
}

extern "C" {

int poms_vec_fill(poms_ctx* ctx, const poms_layout* L, double v, double* z, void* stream) {
    if (!z) { set_error("fill: null vector"); return 1; }
    return vec_common(ctx, L, V_FILL, v, 0.0, nullptr, nullptr, z, nullptr, nullptr, nullptr, stream);
}

int poms_vec_zero_ghosts(poms_ctx* ctx, const poms_layout* L, double* z, void* stream) {
    if (!ctx || !layout_ok(L) || !z) { set_error("zero_ghosts: bad argument"); return 1; }
    zero_ghosts_launch(row_geom(L), z, as_stream(stream));
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_vec_dot(poms_ctx* ctx, const poms_layout* L, const double* x, const double* y,
                 double* out_dev, void* stream) {
    if (!x || !y || !out_dev) { set_error("dot: null argument"); return 1; }
    return vec_common(ctx, L, V_DOT, 0.0, 0.0, x, y, nullptr, nullptr, nullptr, out_dev, stream);
}

int poms_pcg_update(poms_ctx* ctx, const poms_layout* L, double alpha, double* x, const double* p,
                    double* r, const double* q, double* out_dev, void* stream) {
    if (!x || !p || !r || !q || !out_dev) { set_error("pcg_update: null argument"); return 1; }
    return vec_common(ctx, L, V_PCGUPD, alpha, 0.0, nullptr, p, x, r, q, out_dev, stream);
}

int poms_pcg_r_update(poms_ctx* ctx, const poms_layout* L, double alpha, double* r, const double* q,
                      double* out_dev, void* stream) {
    if (!r || !q || !out_dev) { set_error("pcg_r_update: null argument"); return 1; }
    return vec_common(ctx, L, V_RUPD, alpha, 0.0, nullptr, nullptr, nullptr, r, q, out_dev, stream);
}

int poms_pcg_xp_update(poms_ctx* ctx, const poms_layout* L, double alpha, double beta, double* x,
                       double* p, const double* s, void* stream) {
    if (!x || !p || !s) { set_error("pcg_xp_update: null argument"); return 1; }
    return vec_common(ctx, L, V_XPUPD, alpha, beta, s, nullptr, x, p, nullptr, nullptr, stream);
}

// Device-coefficient forms: the scalars are read by the kernel from device memory
// (ab_dev[0], ab_dev[1]), so pcg's alpha / beta never visit the host.
int poms_vec_axpby_dev(poms_ctx* ctx, const poms_layout* L, const double* ab_dev, const double* x,
                       const double* y, double* z, void* stream) {
    if (!x || !y || !z || !ab_dev) { set_error("axpby_dev: null argument"); return 1; }
    return vec_common(ctx, L, V_AXPBY, 0.0, 0.0, x, y, z, nullptr, nullptr, nullptr, stream, ab_dev);
}

int poms_pcg_r_update_dev(poms_ctx* ctx, const poms_layout* L, const double* alpha_dev, double* r,
                          const double* q, double* out_dev, void* stream) {
    if (!r || !q || !out_dev || !alpha_dev) { set_error("pcg_r_update_dev: null argument"); return 1; }
    return vec_common(ctx, L, V_RUPD, 0.0, 0.0, nullptr, nullptr, nullptr, r, q, out_dev, stream, alpha_dev);
}

int poms_pcg_xp_update_dev(poms_ctx* ctx, const poms_layout* L, const double* ab_dev, double* x, double* p,
                           const double* s, void* stream) {
    if (!x || !p || !s || !ab_dev) { set_error("pcg_xp_update_dev: null argument"); return 1; }
    return vec_common(ctx, L, V_XPUPD, 0.0, 0.0, s, nullptr, x, p, nullptr, nullptr, stream, ab_dev);
}

int poms_pcg_p_update_dev(poms_ctx* ctx, const poms_layout* L, const double* ab_dev, const double* s,
                          const double* p, double* p_next, void* stream) {
    if (!ctx || !layout_ok(L) || !s || !p || !p_next || !ab_dev) { set_error("pcg_p_update_dev: bad argument"); return 1; }
    const FlatRange fr = flat_range(row_geom(L));
    int nb = 0;
    if ((L->flags & POMS_LAYOUT_GHOST_DATA) ||
        vec_flat_launch(V_PUPD, fr.count, 0.0, 0.0, s + fr.off, p + fr.off, p_next + fr.off, nullptr, nullptr, nullptr,
                        as_stream(stream), &nb, ab_dev)) {
        set_error("pcg_p_update_dev: needs whole interior planes and one 16-B phase");
        return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

// pcg's last iteration when what follows it is discarded (poms_pcg_opts.skip_tail):
// x += alpha p with V_XPUPD's statement, (r - alpha q).(r - alpha q) with V_RUPD's.
// r - alpha q is not kept: r's buffer takes x as the early-stop update would have
// rounded it (vec_ops.hip: stop_update), for the caller whose stop test then fires
int poms_pcg_final_update_dev(poms_ctx* ctx, const poms_layout* L, const double* alpha_dev, double* x,
                              const double* p, double* r, const double* q, double* out_dev, void* stream) {
    if (!x || !p || !r || !q || !out_dev || !alpha_dev) { set_error("pcg_final_update_dev: null argument"); return 1; }
    return vec_common(ctx, L, V_FINUPD, 0.0, 0.0, nullptr, p, x, r, q, out_dev, stream, alpha_dev);
}

int poms_reduce_partials(poms_ctx* ctx, int64_t count, double* out_dev, void* stream) {
    return poms_reduce_partials_at(ctx, 0, count, out_dev, stream);
}

int poms_reduce_partials_at(poms_ctx* ctx, int64_t offset, int64_t count, double* out_dev, void* stream) {
    if (!ctx || !out_dev || count < 0 || offset < 0 || offset + count > kScratch) {
        set_error("reduce: bad argument");
        return 1;
    }
    reduce_launch(ctx->scratch + offset, (int)count, out_dev, as_stream(stream));
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

// Async copy of `count` doubles from device memory to (pinned) host memory.
int poms_copy_to_host_async(poms_ctx* ctx, const double* src_dev, double* dst_host, int64_t count, void* stream) {
    if (!ctx || !src_dev || !dst_host || count < 0) { set_error("poms_copy_to_host_async: bad argument"); return 1; }
    POMS_HIP_CHECK(hipMemcpyAsync(dst_host, src_dev, count * sizeof(double), hipMemcpyDeviceToHost,
                                  as_stream(stream)));
    return 0;
}

}  // extern "C"
