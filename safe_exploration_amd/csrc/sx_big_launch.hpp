// Launchers of the large-N path (sx_big.hpp: Kstar in HBM, for training sets beyond the LDS budget of the single-launch
// kernels), which sx_gp_predict and sx_cem_rollout share.  Their instantiations -- every shift-0 shape of
// SX_ROLLOUT_SHAPES -- are compiled in a translation unit of their own (sx_big.hip), so that each of its kernels exists
// once; sx_gp_predict.hip and sx_gp_rollout.hip see the declarations.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sx_amd.h"
#include "sx_rollout.hpp"

#include <cstdint>
#include <vector>

namespace sx {

// The A/B settings of trmm_reduce_kernel's launch (SX_TRMM_ORDER / SX_TRMM_VARIANT / SX_TRMM_PT, read once per process by
// trmm_override() in sx_big.hip)
struct TrmmOverride {
    int order;     // tile order bits, or < 0: the launcher's choice
    int variant;   // <pairs per chunk><LDS buffers> of the 128 x 128 tiles: 13 (default), 12, 22, 23
    int pt;        // particle tiles per workgroup, 8 | 4, or 0: the launcher's choice
};
constexpr TrmmOverride kNoTrmmOverride{-1, 13, 0};

// How trmm_reduce_kernel tiles a launch: its instantiation <PPC, NBUF, PT>, the tile order it is handed and its grid.
struct BigTiling {
    int pt, ppc, nbuf;   // particle tiles (of 16) per workgroup; fragment pairs per K-chunk; LDS buffers
    int order;           // 16 paired tiles, 8 longest first, 1 XCD-contiguous, 0 plain (+ 2 / + 4: timing-only diagnostics)
    int row_tiles;       // 128-row tiles of the padded W
    int64_t grid;        // workgroups
    int variant() const { return 10 * ppc + nbuf; }
};

// The tiling of n_s outputs over n_pad rows of W and p128 particles (a multiple of 128), decided here only: launch_trmm
// launches it, sx_gp_big_tiling reports it.  Pure host arithmetic, no HIP call.
inline BigTiling plan_big_tiling(int ns, int n_pad, int64_t p128, const TrmmOverride& o = kNoTrmmOverride) {
    constexpr int kTile = 128, kRb = kTile / 16;   // kBigTile, kBigRb of sx_big.hpp
    BigTiling t;
    t.row_tiles = (n_pad + kTile - 1) / kTile;
    const int row_tiles = t.row_tiles;
    // Small grids take 128 x 64 tiles: with 128 x 128 a grid of up to two workgroups per compute unit (N ~ 1000 .. 1400 at
    // 4096 particles) leaves each SIMD one or two waves that idle through every barrier and DMA wait; twice the workgroups
    // at half the size fill those gaps (tools/n_sweep.sh: the step at the path switch).
    const int64_t wgs8 = (p128 / kTile) * row_tiles * ns;
    const bool half = o.pt ? o.pt == 4 : wgs8 <= 2 * 768;
    t.pt = half ? 4 : 8;
    t.ppc = (!half && (o.variant == 22 || o.variant == 23)) ? 2 : 1;
    t.nbuf = (!half && (o.variant == 12 || o.variant == 22)) ? 2 : 3;
    const int64_t pgroups = p128 / (t.pt * 16);
    const int64_t tiles = pgroups * row_tiles * ns;
    // Tile order.  A large grid runs longest tile first.  A grid of a few rounds is all quantisation: it runs PAIRED tiles
    // (row tile rt and row_tiles - 1 - rt in one workgroup: equal work) when that deals the work out more evenly than
    // longest-first does -- judged by dealing the workgroups round-robin onto the 256 CUs and comparing the fullest CU.
    // SX_TRMM_ORDER overrides.
    int order = o.order;
    if (order < 0) {
        order = 8;
        if (tiles <= 3 * 768 && row_tiles > 1) {
            const int nrb = n_pad >> 4, groups = (int)pgroups * ns;
            std::vector<double> work(row_tiles);
            for (int rt = 0; rt < row_tiles; ++rt) {
                const int rb0 = rt * kRb, rb_end = rb0 + kRb < nrb ? rb0 + kRb : nrb;
                double w = 0.0;
                for (int rb = rb0; rb < rb0 + kRb; ++rb) w += 2 * (rb + 1) < 2 * rb_end ? 2 * (rb + 1) : 2 * rb_end;
                work[rt] = w;
            }
            auto fullest = [&](const std::vector<double>& per_wg) {     // per_wg: work of the workgroups in dispatch order
                double cu[256] = {0.0};
                for (size_t i = 0; i < per_wg.size(); ++i) cu[i & 255] += per_wg[i];
                double m = 0.0;
                for (double v : cu) m = v > m ? v : m;
                return m;
            };
            std::vector<double> plain, paired;
            for (int rt = row_tiles - 1; rt >= 0; --rt) plain.insert(plain.end(), groups, work[rt]);
            for (int j = 0; j < (row_tiles + 1) / 2; ++j)
                paired.insert(paired.end(), groups, work[row_tiles - 1 - j] + (j != row_tiles - 1 - j ? work[j] : 0.0));
            if (fullest(paired) < fullest(plain)) order = 16;
        }
    }
    t.order = order;
    t.grid = (order & 16) ? pgroups * ((row_tiles + 1) / 2) * ns : tiles;
    return t;
}

// sx_gp_predict over `workspace` (big_ws_layout doubles for P points; SX_ERR_ARG if absent or too small)
template <int NS, int NU>
int launch_predict_big(const sx_gp_model* m, const double* z, int P, double* mean, double* var, double* jac,
                       double* workspace, int64_t workspace_bytes, hipStream_t stream);

// sx_cem_rollout over `workspace` (big_ws_layout doubles for E P particles): three launches per step
template <int NS, int NU>
int launch_rollout_big(const sx_gp_model* m, const sx_env* env, const RolloutPtrs& rp, double* workspace,
                       int64_t workspace_bytes, hipStream_t stream);

}  // namespace sx
