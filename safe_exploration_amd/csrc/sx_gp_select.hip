// sx_gp_select: the max-variance subset of a pool of training inputs, E problems side by side (sx_gp_select.hpp).  One
// init launch per kSelInitChunk problems, then one plain launch per greedy step; everything goes on the caller's stream and
// nothing is waited for.  Every argument check answers before the first HIP call (tests/test_subset_select_host.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/sx_amd.h"
#include "sx_gp_select.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"

namespace sx {

template <int NS>
static void launch_select_steps(const SelectArgs& a, dim3 grid, hipStream_t s) {
    for (int j = 0; j < a.m; ++j) hipLaunchKernelGGL(gp_select_step_kernel<NS>, grid, dim3(kSelRows), 0, s, a, j);
}

}  // namespace sx

extern "C" {

int64_t sx_gp_select_workspace_bytes(int n_s, int E, int n_max, int m) {
    if (n_s <= 0 || n_s > SX_MAX_NS || E <= 0 || n_max <= 0 || m <= 0 || m > n_max) return -1;
    if (n_max > sx::kSelMaxN || m > sx::kSelMaxM) return -1;
    return sx::SelectLayout(n_s, E, n_max, m).total;
}

int sx_gp_select(const sx_gp_model* models, int E, int m, const int32_t* seed_idx, int n_seed, int32_t* idx,
                 double* sel_var, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!models || !idx || !sel_var || !status || !workspace) return SX_ERR_ARG;
    if (E <= 0 || m <= 0 || n_seed < 0 || n_seed > m || (n_seed > 0 && !seed_idx)) return SX_ERR_ARG;
    const int ns = models[0].n_s, nu = models[0].n_u;
    if (ns <= 0 || ns > SX_MAX_NS || nu <= 0 || nu > SX_MAX_D - ns) return SX_ERR_ARG;
    int n_max = 0;
    for (int e = 0; e < E; ++e) {
        const sx_gp_model& g = models[e];
        if (g.n_s != ns || g.n_u != nu || g.n_train <= 0 || !g.x_train || m > g.n_train) return SX_ERR_ARG;
        n_max = std::max(n_max, g.n_train);
    }
    if (m > sx::kSelMaxM || n_max > sx::kSelMaxN || E > 65535) return SX_ERR_UNSUPPORTED;   // (E: the grid's y limit)
    const sx::SelectLayout lay(ns, E, n_max, m);
    if (workspace_bytes < lay.total) return SX_ERR_ARG;

    sx::SelectArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ws = static_cast<char*>(workspace);
    a.seed_idx = n_seed > 0 ? seed_idx : nullptr;
    a.idx = idx;
    a.sel_var = sel_var;
    a.status = status;
    a.E = E;
    a.n_s = ns;
    a.D = ns + nu;
    a.n_max = n_max;
    a.m = m;
    a.n_seed = n_seed;
    hipStream_t s = (hipStream_t)stream;
    for (int e0 = 0; e0 < E; e0 += sx::kSelInitChunk) {
        const int count = std::min(sx::kSelInitChunk, E - e0);
        sx::SelectInitArgs ia;
        std::memset(&ia, 0, sizeof(ia));
        ia.e0 = e0;
        for (int k = 0; k < count; ++k) {
            const sx_gp_model& g = models[e0 + k];
            sx::copy_hyper(g, ia.entry[k].inv_ls2, ia.entry[k].outputscale, ia.entry[k].noise);
            ia.entry[k].x = g.x_train;
            ia.entry[k].n = g.n_train;
        }
        hipLaunchKernelGGL(sx::gp_select_init_kernel, dim3(lay.nwg, count), dim3(sx::kSelRows), 0, s, a, ia);
    }
    const dim3 grid(lay.nwg, E);
    switch (ns) {
        case 1: sx::launch_select_steps<1>(a, grid, s); break;
        case 2: sx::launch_select_steps<2>(a, grid, s); break;
        case 3: sx::launch_select_steps<3>(a, grid, s); break;
        default: sx::launch_select_steps<4>(a, grid, s); break;
    }
    return sx::check_launch();
}

}  // extern "C"
