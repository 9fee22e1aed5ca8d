// Ranking and hand-off: the ranking kernels of sx_rank.hpp and sx_rank_count.hpp, pack_result_kernel, and the entries
// sx_cem_rank_counts, sx_cem_rank_refit and sx_cem_pack_result.  The diagnostic build's sx_debug_set_stamps sets this
// translation unit's stamp buffer, the one the ranking kernels write (tools/rank_stamps.py).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>

#include "../../include/sx_amd.h"
#include "sx_launch.hpp"
#include "sx_rank.hpp"
#include "sx_rank_count.hpp"

#ifdef SX_STAMPS
namespace sx {
unsigned long long* g_stamp_host = nullptr;   // the phase-stamp buffer; sx_gp_rollout.hip hands it to the rollout launchers
}

extern "C" int sx_debug_set_stamps(unsigned long long* dev_buf) {
    sx::g_stamp_host = dev_buf;
    return hipMemcpyToSymbol(HIP_SYMBOL(sx::g_stamp_buf), &dev_buf, sizeof(dev_buf)) == hipSuccess ? SX_OK : SX_ERR_LAUNCH;
}
#endif

extern "C" {

// (inside extern "C": the kernel's symbol is the unmangled pack_result_kernel, which profiles and kernel statistics name)
namespace sx {
// sx_cem_pack_result: one small workgroup
__global__ __launch_bounds__(256) void pack_result_kernel(int G, int E, int L, const int* __restrict__ status,
                                                          const int* __restrict__ best_ok, const double* __restrict__ q_block,
                                                          long long q_count, const double* __restrict__ best,
                                                          double* __restrict__ out) {
    __shared__ int any_nz;
    const int tid = threadIdx.x;
    if (tid == 0) any_nz = 0;
    __syncthreads();
    int nz = 0;
    if (q_block)
        for (long long i = tid; i < q_count; i += blockDim.x) nz |= (q_block[i] != 0.0) ? 1 : 0;   // (NaN counts as non-zero)
    if (nz) atomicOr(&any_nz, 1);
    for (int i = tid; i < G; i += blockDim.x) out[i] = (double)status[i];
    for (int i = tid; i < E; i += blockDim.x) out[G + i] = (double)best_ok[i];
    for (int i = tid; i < E * L; i += blockDim.x) out[G + E + 1 + i] = best[i];
    __syncthreads();
    if (tid == 0) out[G + E] = any_nz ? 1.0 : 0.0;
}
}  // namespace sx

int sx_cem_pack_result(int G, int E, int row_len, const int32_t* status, const int32_t* best_ok, const double* q_block,
                       int64_t q_count, const double* best, double* out, void* stream) {
    if (G <= 0 || E <= 0 || row_len <= 0 || !status || !best_ok || !best || !out || q_count < 0) return SX_ERR_ARG;
    hipLaunchKernelGGL(sx::pack_result_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, G, E, row_len, status, best_ok,
                       q_count > 0 ? q_block : nullptr, (long long)q_count, best, out);
    return sx::check_launch();
}

// Which ranking kernel: by shape only (every rank of a multi-GPU solve must take the same one: the elite order differs).
// Counting spreads one or two problems over the chip (E P / 16 workgroups, all keys in each one's LDS); many problems at
// once already fill it with the one-workgroup kernel (SX_RANK_PATH = count | select overrides, for A/B measurements).
int sx_cem_rank_counts(int E, int P) {
    if (E <= 0 || P <= 0 || P > sx::kCountMaxP || E > sx::kCountMaxE) return 0;
    static const char* const forced = std::getenv("SX_RANK_PATH");
    if (forced && forced[0] == 's') return 0;
    if (forced && forced[0] == 'c') return 1;
    return (long long)E * ((P + 15) / 16) <= sx::kCountMaxGrid ? 1 : 0;
}

int sx_cem_rank_refit(int E, int P, int k, int row_len, const double* con_cost, const double* obj_cost,
                      int64_t cost_stride, const double* actions, int64_t act_stride, int32_t* elite_idx,
                      double* elite_rows, double* mean, double* std, double* best, int32_t* best_ok, void* stream) {
    if (!con_cost || !obj_cost || !actions || E <= 0 || P <= 0 || k <= 0 || row_len <= 0) return SX_ERR_ARG;
    if (k > P) return SX_ERR_ARG;
    if (k > sx::kRankMaxK) return SX_ERR_UNSUPPORTED;
    sx::RankArgs ra{P,      k,          row_len,    con_cost, obj_cost, (long long)cost_stride,
                    actions, (long long)act_stride, elite_idx, elite_rows, mean,     std,
                    best,   best_ok};
    const bool count = sx_cem_rank_counts(E, P) != 0 && (elite_rows || !mean);
    const int tiles = (P + 15) / 16;
    if (count) {
        const size_t lds = (size_t)((P + 127) & ~127) * sizeof(sx::CountKey);
        if (int rc = sx::allow_lds(sx::cem_rank_count_kernel, lds)) return rc;
        // the refit's ticket cells: one set per launch, kCountTicketSlots sets in rotation (launches whose refits overlap in
        // time must be fewer than that); the symbol's address is looked up once per device
        static std::atomic<unsigned int> seq{0};
        unsigned int* tickets = nullptr;
        if (mean) {
            static std::mutex mu;
            static std::map<int, unsigned int*> base;
            int dev = 0;
            (void)hipGetDevice(&dev);
            std::lock_guard<std::mutex> lock(mu);
            auto it = base.find(dev);
            if (it == base.end()) {
                unsigned int* p = nullptr;
                if (hipGetSymbolAddress((void**)&p, HIP_SYMBOL(sx::g_rank_tickets)) != hipSuccess) return SX_ERR_LAUNCH;
                it = base.emplace(dev, p).first;
            }
            tickets = it->second + (size_t)(seq.fetch_add(1) % sx::kCountTicketSlots) * sx::kCountMaxE;
        }
        sx::launch(SX_PROF_RANK, sx::cem_rank_count_kernel, dim3((unsigned)tiles, (unsigned)E), dim3(sx::kCountThreads), lds,
                   (hipStream_t)stream, ra, tickets);
        return sx::check_launch();
    }
    if (P > sx::kRankThreads * sx::kRankSlots) return SX_ERR_UNSUPPORTED;
    const int slots = (P + sx::kRankThreads - 1) / sx::kRankThreads;
    if (slots <= 4)
        sx::launch(SX_PROF_RANK, sx::cem_rank_kernel<4>, dim3(E), dim3(sx::kRankThreads), 0, (hipStream_t)stream, ra);
    else if (slots <= 8)
        sx::launch(SX_PROF_RANK, sx::cem_rank_kernel<8>, dim3(E), dim3(sx::kRankThreads), 0, (hipStream_t)stream, ra);
    else
        sx::launch(SX_PROF_RANK, sx::cem_rank_kernel<sx::kRankSlots>, dim3(E), dim3(sx::kRankThreads), 0, (hipStream_t)stream, ra);
    return sx::check_launch();
}

}  // extern "C"
