// sx_sat_cost_eval: the saturating cost alone (sx_sat_cost.hpp), one particle per lane, for n_s = 1 .. SX_MAX_NS.
#include "sx_host.hpp"
#include "sx_launch.hpp"
#include "sx_sat_cost.hpp"

namespace sx {

template <int NS>
static int sat_cost_eval(const sx_sat_cost* cost, int P, const double* mu, const double* cov, double* loss, int32_t* status,
                         hipStream_t stream) {
    SatConst<NS> k;
    make_sat_const<NS>(cost, k);
    const unsigned blocks = (unsigned)(((int64_t)P + 255) / 256);
    hipLaunchKernelGGL(sat_cost_eval_kernel<NS>, dim3(blocks), dim3(256), 0, stream, k, P, mu, cov, loss, status);
    return check_launch();
}

}  // namespace sx

extern "C" int sx_sat_cost_eval(const sx_sat_cost* cost, int n_s, int P, const double* mu, const double* cov, double* loss,
                                int32_t* status, void* stream) {
    if (!cost || !mu || !cov || !loss || !status || P <= 0) return SX_ERR_ARG;
    if (!sx::sat_cost_ok(cost, n_s)) return SX_ERR_ARG;
    switch (n_s) {
        case 1: return sx::sat_cost_eval<1>(cost, P, mu, cov, loss, status, (hipStream_t)stream);
        case 2: return sx::sat_cost_eval<2>(cost, P, mu, cov, loss, status, (hipStream_t)stream);
        case 3: return sx::sat_cost_eval<3>(cost, P, mu, cov, loss, status, (hipStream_t)stream);
        default: return sx::sat_cost_eval<4>(cost, P, mu, cov, loss, status, (hipStream_t)stream);
    }
}
