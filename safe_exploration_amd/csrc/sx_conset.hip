// sx_conset_eval: the constraint set's cost of one step alone (sx_conset.hpp), one particle per lane, for every
// (n_s, n_u) up to (SX_MAX_NS, SX_MAX_NU).
#include "sx_conset.hpp"
#include "sx_host.hpp"
#include "sx_launch.hpp"

namespace sx {

template <int NS, int NU>
static int conset_eval(const sx_env* env, const sx_con_set* cons, int P, const double* u, const double* q_start,
                       const double* p_next, const double* q_next, int check_obstacle, double* con_step,
                       hipStream_t stream) {
    ReachConst<NS, NU> rc;
    CostConst<SX_MAX_M, NS, NU> cc;
    if (!make_reach_const<NS, NU>(env, rc)) return SX_ERR_ARG;
    make_cost_const<NS, NU>(env, cc);
    ConConst<NS> k;
    make_con_const<NS>(cons, k);
    const unsigned blocks = (unsigned)(((int64_t)P + 255) / 256);
    hipLaunchKernelGGL((conset_eval_kernel<NS, NU>), dim3(blocks), dim3(256), 0, stream, rc, cc, k, P, u, q_start, p_next,
                       q_next, check_obstacle, con_step);
    return check_launch();
}

}  // namespace sx

extern "C" int sx_conset_eval(const sx_env* env, const sx_con_set* cons, int P, const double* u, const double* q_start,
                              const double* p_next, const double* q_next, int check_obstacle, double* con_step,
                              void* stream) {
    if (!env || !cons || !u || !con_step || P <= 0) return SX_ERR_ARG;
    if (env->n_u < 1 || env->n_u > SX_MAX_NU || env->m < 0 || env->m > SX_MAX_M) return SX_ERR_ARG;
    if (!sx::con_set_ok(cons, env->n_s)) return SX_ERR_ARG;
    if (check_obstacle && cons->m_obs > 0 && !(p_next && q_next)) return SX_ERR_ARG;
#define SX_CONSET_CASE(NS, NU) \
    if (env->n_s == NS && env->n_u == NU) \
        return sx::conset_eval<NS, NU>(env, cons, P, u, q_start, p_next, q_next, check_obstacle, con_step, (hipStream_t)stream);
    SX_CONSET_CASE(1, 1) SX_CONSET_CASE(2, 1) SX_CONSET_CASE(3, 1) SX_CONSET_CASE(4, 1)
    SX_CONSET_CASE(1, 2) SX_CONSET_CASE(2, 2) SX_CONSET_CASE(3, 2) SX_CONSET_CASE(4, 2)
#undef SX_CONSET_CASE
    return SX_ERR_ARG;
}
