// extern "C" boundary of libpoms_hip.so (declared in include/poms_hip.h): block vector
// algebra on lists of padded vectors, the Gram matrix and linear combinations.
#include "common.hpp"
#include "launchers.hpp"
#include "abi_internal.hpp"
#include "../../include/poms_hip.h"

using namespace poms;

static_assert(kBlockMax == POMS_BLOCK_MAX, "the header's list limit is the kernels'");

// every pointer of a list present and a whole number of doubles into memory
static bool list_ok(const double* const* v, int n) {
    if (!v) return false;
    for (int k = 0; k < n; ++k)
        if (!v[k] || (reinterpret_cast<uintptr_t>(v[k]) & 7)) return false;
    return true;
}

extern "C" {

int poms_block_gram(poms_ctx* ctx, const poms_layout* L, int nx, const double* const* xs, int ny,
                    const double* const* ys, int symmetric, double* out_dev, void* stream) {
    if (!ctx || !layout_ok(L) || !out_dev) { set_error("block_gram: bad context, layout or output"); return 1; }
    if (nx < 1 || ny < 1 || nx > kBlockMax || ny > kBlockMax) {
        set_error("block_gram: 1 to POMS_BLOCK_MAX vectors per list");
        return 1;
    }
    if (symmetric && nx != ny) { set_error("block_gram: a symmetric result needs nx == ny"); return 1; }
    if (!list_ok(xs, nx) || !list_ok(ys, ny)) { set_error("block_gram: null or misaligned vector"); return 1; }
    if (L->flags & POMS_LAYOUT_GHOST_DATA) {
        set_error("block_gram: a layout whose ghost rows hold data (POMS_LAYOUT_GHOST_DATA) is not supported");
        return 1;
    }
    const FlatRange fr = flat_range(row_geom(L));
    const double *xo[kBlockMax], *yo[kBlockMax];
    for (int k = 0; k < nx; ++k) xo[k] = xs[k] + fr.off;
    for (int k = 0; k < ny; ++k) yo[k] = ys[k] + fr.off;
    if (block_gram_launch(fr.count, nx, xo, ny, yo, symmetric ? 1 : 0, ctx->scratch, out_dev, as_stream(stream))) {
        set_error("block_gram: nothing launched");
        return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_block_combine(poms_ctx* ctx, const poms_layout* L, int nin, const double* const* ins, int nout,
                       double* const* outs, const double* coef_dev, void* stream) {
    if (!ctx || !layout_ok(L) || !coef_dev) { set_error("block_combine: bad context, layout or coefficients"); return 1; }
    if (nin < 1 || nin > kBlockMax || nout < 1 || nout > kCombineMaxOut) {
        set_error("block_combine: 1 to POMS_BLOCK_MAX inputs and 1 to 16 outputs");
        return 1;
    }
    if (!list_ok(ins, nin) || !list_ok(outs, nout)) { set_error("block_combine: null or misaligned vector"); return 1; }
    if (L->flags & POMS_LAYOUT_GHOST_DATA) {
        set_error("block_combine: a layout whose ghost rows hold data (POMS_LAYOUT_GHOST_DATA) is not supported");
        return 1;
    }
    for (int j = 0; j < nout; ++j) {
        for (int i = 0; i < nin; ++i)
            if (outs[j] == ins[i]) { set_error("block_combine: an output is also an input"); return 1; }
        for (int k = 0; k < j; ++k)
            if (outs[j] == outs[k]) { set_error("block_combine: two outputs are the same vector"); return 1; }
    }
    const FlatRange fr = flat_range(row_geom(L));
    const double* io[kBlockMax];
    double* oo[kCombineMaxOut];
    for (int k = 0; k < nin; ++k) io[k] = ins[k] + fr.off;
    for (int k = 0; k < nout; ++k) oo[k] = outs[k] + fr.off;
    if (block_combine_launch(fr.count, nin, io, nout, oo, coef_dev, as_stream(stream))) {
        set_error("block_combine: nothing launched");
        return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
