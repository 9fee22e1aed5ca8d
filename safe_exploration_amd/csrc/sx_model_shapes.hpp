// The shapes of the fused junk-dimension rollout over feature-GP and MC-dropout models (sx_cem_rollout_feat_junk,
// sx_cem_rollout_mlp_junk) and the dispatch over them; sx_feat.hip and sx_mlp.hip instantiate their kernels from it.
#pragma once
#include "sx_stream_launch.hpp"   // SX_DISPATCH

// (n_s, n_u, query shift > 0) of sx_cem_rollout_feat_junk and sx_cem_rollout_mlp_junk: X(NS, NU, SH, ...) for every shape a
// padded feature-GP or MC-dropout model can be built for (n_s + J_s <= SX_MAX_NS, n_u + J_a <= SX_MAX_NU, SH = min(J_s, n_u));
// shift 0 is the shapes of sx_cem_rollout_feat / sx_cem_rollout_mlp.  ssm_cem.JUNK_MODEL_FUSED_SHAPES mirrors this list.
#define SX_MODEL_JUNK_SHAPES(X, ...)                                                                                    \
    X(1, 1, 1, __VA_ARGS__) X(2, 1, 1, __VA_ARGS__) X(3, 1, 1, __VA_ARGS__) X(2, 2, 1, __VA_ARGS__)                     \
    X(2, 2, 2, __VA_ARGS__) X(3, 2, 1, __VA_ARGS__)
// return CALL(NS, NU, SH) for the shape (ns, nu, sh): SX_DISPATCH's shapes with SH = 0 for sh = 0, the list above else
#define SX_MODEL_JUNK_ONE(NS, NU, SH, ns, nu, sh, CALL) \
    if ((ns) == NS && (nu) == NU && (sh) == SH) return CALL(NS, NU, SH);
#define SX_MODEL_JUNK_DISPATCH(ns, nu, sh, CALL)                             \
    do {                                                                     \
        if ((sh) == 0) {                                                     \
            SX_DISPATCH(ns, nu, CALL##_0);                                   \
        }                                                                    \
        SX_MODEL_JUNK_SHAPES(SX_MODEL_JUNK_ONE, ns, nu, sh, CALL)            \
        return SX_ERR_UNSUPPORTED;                                           \
    } while (0)

namespace sx {

// query shift 0 .. env->n_u; the model over n_s + n_u + shift columns (the plain model for shift 0)
inline bool junk_env_ok(const sx_env* env, int model_ns, int model_nu, int query_shift) {
    if (!env || env->n_s <= 0 || env->n_s > SX_MAX_NS || env->n_u <= 0 || env->n_u > SX_MAX_NU) return false;
    if (query_shift < 0 || query_shift > env->n_u) return false;
    return model_ns == env->n_s && model_nu == env->n_u + query_shift;
}

}  // namespace sx
