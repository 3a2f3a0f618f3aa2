// GradPlanner for MI355X (gfx950): gradient trajectory planning by the adjoint
// of the gym step (the law is restated in NumPy by
// tests/gplan_ref.py, one numpy call per operation below, in this order).
//
// One thread per env.  The env's 15 state words, the running adjoint (12
// words) and the two states an adjoint step sits between live in registers;
// what a runtime h indexes -- the action sequence U, Adam's m and s and the
// tape of the states between the steps -- lives in the caller's workspace,
// word-major ([word][env]), so a wave reads and writes contiguous runs.
//   forward   H steps of physics_step<double, DR_VARIANT_GYM>, the function
//             the env kernels call, on a_h = clip(U[h]); the state before
//             step h >= 1 goes to the tape, the cost accumulates
//   backward  h = H - 1 .. 0: the step's direct cost gradient joins the
//             adjoint, gym_step_adjoint carries it to the state before the
//             step (sin / cos recomputed from the taped Euler angles), and
//             dc/dU[h] feeds Adam at once: U[h], m[h], s[h] are touched by
//             no other step, so the gradient itself is never stored
// `iterations` such sweeps per launch.  No atomics, no LDS, no cross-lane
// traffic: every env's result depends on its own inputs alone and reruns and
// graph replays are bitwise equal.
//
// Built as part of env_kernels.hip's translation unit, the one place where the
// model function is visible.  Every name at namespace scope here carries a
// gp / Gp prefix, but for gym_step_adjoint and gym_step_action_grad, which a
// later trainer is meant to call.

#include <cmath>
#include <string>

#include "common.h"

#pragma clang fp contract(off)

namespace dr {
namespace {

constexpr int kGpMaxH = DR_GPLAN_MAX_HORIZON;
constexpr int kGpMaxIter = DR_GPLAN_MAX_ITERATIONS;
// One wave per block: below 65,536 envs the grid has fewer waves than the chip
// has SIMDs, so the smallest block spreads them over the most CUs, and a lone
// wave may use the whole 512-entry register file.
constexpr int kGpBlock = 64;
constexpr int kGpTape = 12;              // p, v, euler, omega of the state before a step

int gp_fail(const std::string &msg) {
    set_global_error(msg);
    return DR_ERR_INVALID;
}

// Words of the workspace, each an array of n: m and s (4 H f64 each), the tape
// (12 (H - 1) f64: the start state stays in registers), then U (4 H f32).
inline size_t gp_workspace_bytes(int64_t n, int H) {
    return (size_t)n * ((size_t)(8 * H + kGpTape * (H - 1)) * sizeof(double) +
                        (size_t)(4 * H) * sizeof(float));
}

struct GpArgs {
    int64_t n;
    int H, I;
    double lr, b1, b2, omb1, omb2, eps;       // omb = 1 - beta, rounded on the host
    double w_pos, w_vel, w_att, w_rate, w_eff, w_pf, w_vf;
    const float *obs;
    const uint8_t *dones;      // nullable
    float *nominal;            // (n, H, 4)
    double *m, *s, *tape;      // the workspace's parts
    float *U;
    float *actions;            // (n, 4)
    double *cost;              // (n,), nullable
    double *grad;              // (n, H, 4), nullable
    double pw1[kGpMaxIter];    // beta1^it, it = 1 ..
    double pw2[kGpMaxIter];
};

__device__ inline double gp_sq3(double x, double y, double z) { return (x * x + y * y) + z * z; }

// The adjoint (reverse-mode derivative) of one gym step of physics_step_mixed
// on the nominal airframe in still air, dt = kDt.  sn / cs: sin and cos of the
// Euler angles before the step; w: omega before the step; T: (double) of the
// f32 thrust sum.  In: the adjoint (lp, lv, le, lw) of the state after the
// step, the step's direct cost gradient already added.  Out: in their place
// the adjoint of the state before the step; gT = dc/dT and nu_k = lw_k dt /
// I_k, from which gym_step_action_grad forms dc/da.
__device__ inline void gym_step_adjoint(const double sn[3], const double cs[3], const double w[3],
                                        double T, double lp[3], double lv[3], double le[3],
                                        double lw[3], double &gT, double nu[3]) {
    const double sph = sn[0], sth = sn[1], sps = sn[2];
    const double cph = cs[0], cth = cs[1], cps = cs[2];
    const double w0 = w[0], w1 = w[1], w2 = w[2];
    constexpr double dt = kDt;
    constexpr double c_yz = kIyy - kIzz, c_zx = kIzz - kIxx, c_xy = kIxx - kIyy;
    const double sec = 1.0 / cth;
    const double tth = sth * sec;
    const double sg = sph * w1 + cph * w2;
    const double ed1 = cph * w1 - sph * w2;
    const double r02 = cps * sth * cph + sps * sph;
    const double r12 = sps * sth * cph - cps * sph;
    const double r22 = cth * cph;
    // p' = p + v' dt, v' = v + acc dt: lp passes through, lv collects lp dt
    const double lvt0 = lv[0] + lp[0] * dt, lvt1 = lv[1] + lp[1] * dt, lvt2 = lv[2] + lp[2] * dt;
    const double q0 = lvt0 * dt, q1 = lvt1 * dt, q2 = lvt2 * dt;
    gT = ((r02 * q0 + r12 * q1) + r22 * q2) / kMass;
    const double Tm = T / kMass;
    const double A0 = Tm * (((-cps * sth * sph + sps * cph) * q0 +
                             (-sps * sth * sph - cps * cph) * q1) + (-cth * sph) * q2);
    const double A1 = Tm * (((cps * cth * cph) * q0 + (sps * cth * cph) * q1) +
                            (-sth * cph) * q2);
    const double A2 = Tm * (-r12 * q0 + r02 * q1);
    const double mu0 = le[0] * dt, mu1 = le[1] * dt, mu2 = le[2] * dt;
    const double le0 = (le[0] + A0) + ((mu0 * ed1 * tth - mu1 * sg) + mu2 * ed1 * sec);
    const double le1 = (le[1] + A1) + (mu0 * sg * sec * sec + mu2 * sg * sec * tth);
    const double le2 = le[2] + A2;
    const double nu0 = lw[0] * dt / kIxx, nu1 = lw[1] * dt / kIyy, nu2 = lw[2] * dt / kIzz;
    const double lw0 = (lw[0] + mu0) + (-c_zx * w2 * nu1 - c_xy * w1 * nu2);
    const double lw1 = (lw[1] + ((sph * tth * mu0 + cph * mu1) + sph * sec * mu2)) +
                       (-c_yz * w2 * nu0 - c_xy * w0 * nu2);
    const double lw2 = (lw[2] + ((cph * tth * mu0 - sph * mu1) + cph * sec * mu2)) +
                       (-c_yz * w1 * nu0 - c_zx * w0 * nu1);
    lv[0] = lvt0, lv[1] = lvt1, lv[2] = lvt2;
    le[0] = le0, le[1] = le1, le[2] = le2;
    lw[0] = lw0, lw[1] = lw1, lw[2] = lw2;
    nu[0] = nu0, nu[1] = nu1, nu[2] = nu2;
}

// dc/da_j = gT + F (Sphi_j nu0 + Stheta_j nu1) + K Spsi_j nu2, the sign rows
// motor_mix's: Sphi = (+,+,-,-), Stheta = (-,+,+,-), Spsi = (+,-,+,-).
__device__ inline void gym_step_action_grad(double gT, const double nu[3], double g[4]) {
    constexpr double F = kFactor, K = (double)kKyaw32;
    const double ky = K * nu[2];
    g[0] = (gT + F * (nu[0] - nu[1])) + ky;
    g[1] = (gT + F * (nu[0] + nu[1])) + -ky;
    g[2] = (gT + F * (-nu[0] + nu[1])) + ky;
    g[3] = (gT + F * (-nu[0] - nu[1])) + -ky;
}

__global__ __launch_bounds__(kGpBlock) void gplan_step_kernel(GpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kGpBlock + threadIdx.x;
    const int64_t n = a.n;
    if (i >= n) return;
    const int H = a.H;
    float *const nom = a.nominal + i * (H * 4);
    float *const U = a.U + i;
    double *const M = a.m + i, *const S = a.s + i, *const tape = a.tape + i;

    // the start state the policy's observation describes
    double st0[F_N];
#pragma unroll
    for (int k = 0; k < 12; ++k) st0[k] = (double)a.obs[i * 15 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) st0[F_TGT + k] = st0[k] + (double)a.obs[i * 15 + 12 + k];
    // the nominal (hover where the obs opens a new episode), word-major
    const bool fresh = a.dones && a.dones[i];
    for (int j = 0; j < H * 4; ++j) U[j * n] = fresh ? kHover32 : nom[j];

    const double tw_pos = 2.0 * a.w_pos, tw_vel = 2.0 * a.w_vel, tw_att = 2.0 * a.w_att;
    const double tw_rate = 2.0 * a.w_rate, tw_eff = 2.0 * a.w_eff;
    const double tw_pf = 2.0 * a.w_pf, tw_vf = 2.0 * a.w_vf;
    const double hover = (double)kHover32;
    bool bad = false;
    for (int it = 0; it < a.I; ++it) {
        double st[F_N];
#pragma unroll
        for (int k = 0; k < F_N; ++k) st[k] = st0[k];
        double c = 0.0;
        for (int h = 0; h < H; ++h) {
            if (h > 0) {
#pragma unroll
                for (int k = 0; k < kGpTape; ++k) tape[((h - 1) * kGpTape + k) * n] = st[k];
            }
            const float4 act{pl_clip(U[(4 * h + 0) * n]), pl_clip(U[(4 * h + 1) * n]),
                             pl_clip(U[(4 * h + 2) * n]), pl_clip(U[(4 * h + 3) * n])};
            bool crash;
            physics_step<double, DR_VARIANT_GYM>(st, act, (double)kDt, crash);
            const double d0 = (double)act.x - hover, d1 = (double)act.y - hover;
            const double d2 = (double)act.z - hover, d3 = (double)act.w - hover;
            const double ae = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
            const double dp2 = gp_sq3(st[F_POS] - st[F_TGT], st[F_POS + 1] - st[F_TGT + 1],
                                      st[F_POS + 2] - st[F_TGT + 2]);
            const double v2 = gp_sq3(st[F_VEL], st[F_VEL + 1], st[F_VEL + 2]);
            const double e2 = gp_sq3(st[F_EUL], st[F_EUL + 1], st[F_EUL + 2]);
            const double o2 = gp_sq3(st[F_OMG], st[F_OMG + 1], st[F_OMG + 2]);
            c = c + ((((a.w_pos * dp2 + a.w_vel * v2) + a.w_att * e2) + a.w_rate * o2) +
                     a.w_eff * ae);
        }
        double xn[kGpTape], lp[3], lv[3], le[3], lw[3];
#pragma unroll
        for (int k = 0; k < kGpTape; ++k) xn[k] = st[k];
        {
            const double dx = xn[F_POS] - st0[F_TGT], dy = xn[F_POS + 1] - st0[F_TGT + 1];
            const double dz = xn[F_POS + 2] - st0[F_TGT + 2];
            c = c + (a.w_pf * gp_sq3(dx, dy, dz) +
                     a.w_vf * gp_sq3(xn[F_VEL], xn[F_VEL + 1], xn[F_VEL + 2]));
            lp[0] = tw_pf * dx, lp[1] = tw_pf * dy, lp[2] = tw_pf * dz;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lv[k] = tw_vf * xn[F_VEL + k];
            le[k] = 0.0;
            lw[k] = 0.0;
        }
        if (it == 0) {
            if (a.cost) a.cost[i] = c;
            bad = !(c - c == 0.0);
        }
        const double bc1 = 1.0 - a.pw1[it], bc2 = 1.0 - a.pw2[it];

        for (int h = H - 1; h >= 0; --h) {
            // the direct cost gradient at the state after step h
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lp[k] = lp[k] + tw_pos * (xn[F_POS + k] - st0[F_TGT + k]);
                lv[k] = lv[k] + tw_vel * xn[F_VEL + k];
                le[k] = le[k] + tw_att * xn[F_EUL + k];
                lw[k] = lw[k] + tw_rate * xn[F_OMG + k];
            }
            // the state before it
            double xo[kGpTape];
            if (h > 0) {
#pragma unroll
                for (int k = 0; k < kGpTape; ++k) xo[k] = tape[((h - 1) * kGpTape + k) * n];
            } else {
#pragma unroll
                for (int k = 0; k < kGpTape; ++k) xo[k] = st0[k];
            }
            const float u[4] = {U[(4 * h + 0) * n], U[(4 * h + 1) * n], U[(4 * h + 2) * n],
                                U[(4 * h + 3) * n]};
            const float4 act{pl_clip(u[0]), pl_clip(u[1]), pl_clip(u[2]), pl_clip(u[3])};
            const float ac[4] = {act.x, act.y, act.z, act.w};
            double sn[3], cs[3], gT, nu[3], g[4];
            m_sincos3(&xo[F_EUL], sn, cs);
            gym_step_adjoint(sn, cs, &xo[F_OMG], (double)motor_mix(act).thr, lp, lv, le, lw, gT,
                             nu);
            gym_step_action_grad(gT, nu, g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double gj = g[j] + tw_eff * ((double)ac[j] - hover);
                const int64_t word = (int64_t)(4 * h + j) * n;
                double mj = 0.0, sj = 0.0;
                if (it == 0) {
                    if (a.grad) a.grad[(i * H + h) * 4 + j] = gj;
                    bad = bad || !(gj - gj == 0.0);
                } else {
                    mj = M[word];
                    sj = S[word];
                }
                mj = a.b1 * mj + a.omb1 * gj;
                sj = a.b2 * sj + a.omb2 * (gj * gj);
                const double step = (a.lr * (mj / bc1)) / (m_sqrt(sj / bc2) + a.eps);
                M[word] = mj;
                S[word] = sj;
                U[word] = pl_clip((float)((double)u[j] - step));
            }
#pragma unroll
            for (int k = 0; k < kGpTape; ++k) xn[k] = xo[k];
        }
        // not finite: this env's nominal stays, its later sweeps are void
        if (bad) break;
    }

    // the stores: this call's action and the shifted nominal
    if (!bad) {
        for (int j = 0; j < H * 4; ++j) {
            const float u = U[j * n];
            if (j < 4) a.actions[i * 4 + j] = u;
            else nom[j - 4] = u;
            if (j >= (H - 1) * 4) nom[j] = u;
        }
    } else {
        for (int j = 0; j < H * 4; ++j)
            if (fresh) nom[j] = kHover32;
        for (int j = 0; j < 4; ++j) a.actions[i * 4 + j] = pl_clip(fresh ? kHover32 : nom[j]);
    }
}

__global__ __launch_bounds__(kBlock) void gplan_reset_kernel(int64_t words, float *nominal) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < words) nominal[i] = kHover32;
}

inline bool gp_pos_finite(double x) { return x > 0.0 && std::isfinite(x); }

// The checks both entry points share.
int gp_check(const char *who, const dr_gplan_config *cfg, int64_t n, const float *nominal) {
    const std::string w(who);
    if (!cfg) return gp_fail(w + ": config must be non-null");
    if (n < 1 || n > 0x7fffffff) return gp_fail(w + ": n must be in [1, 2^31)");
    if (cfg->horizon < 1 || cfg->horizon > kGpMaxH)
        return gp_fail(w + ": horizon must be in [1, 32]");
    if (cfg->iterations < 1 || cfg->iterations > kGpMaxIter)
        return gp_fail(w + ": iterations must be in [1, 64]");
    if (!gp_pos_finite(cfg->lr)) return gp_fail(w + ": lr must be > 0 and finite");
    if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0)) return gp_fail(w + ": beta1 must be in [0, 1)");
    if (!(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0)) return gp_fail(w + ": beta2 must be in [0, 1)");
    if (!gp_pos_finite(cfg->adam_eps)) return gp_fail(w + ": adam_eps must be > 0 and finite");
    const struct {
        const char *name;
        double v;
    } weights[] = {{"w_pos", cfg->w_pos}, {"w_vel", cfg->w_vel}, {"w_att", cfg->w_att},
                   {"w_rate", cfg->w_rate}, {"w_effort", cfg->w_effort},
                   {"w_pos_final", cfg->w_pos_final}, {"w_vel_final", cfg->w_vel_final}};
    for (const auto &x : weights)
        if (!pl_nonneg_finite(x.v))
            return gp_fail(w + ": " + x.name + " must be >= 0 and finite");
    if (!nominal) return gp_fail(w + ": nominal must be non-null");
    return DR_OK;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_gplan_workspace_bytes(int64_t n, int32_t horizon) {
    if (n < 1 || n > 0x7fffffff || horizon < 1 || horizon > kGpMaxH) return 0;
    return gp_workspace_bytes(n, horizon);
}

int dr_gplan_reset(const dr_gplan_config *cfg, int64_t n, float *nominal, void *stream) {
    if (int rc = gp_check("dr_gplan_reset", cfg, n, nominal)) return rc;
    const int64_t words = n * cfg->horizon * 4;
    hipLaunchKernelGGL(gplan_reset_kernel, dim3(grid_for(words)), dim3(kBlock), 0,
                       as_stream(stream), words, nominal);
    return launched(nullptr, "dr_gplan_reset");
}

int dr_gplan_step(const dr_gplan_config *cfg, int64_t n, const float *obs, const uint8_t *dones,
                  float *nominal, void *workspace, size_t workspace_bytes, float *actions_out,
                  double *cost_out, double *grad_out, void *stream) {
    if (int rc = gp_check("dr_gplan_step", cfg, n, nominal)) return rc;
    if (!obs) return gp_fail("dr_gplan_step: obs must be non-null");
    if (!actions_out) return gp_fail("dr_gplan_step: actions_out must be non-null");
    if (!workspace) return gp_fail("dr_gplan_step: workspace must be non-null");
    if ((uintptr_t)workspace % sizeof(double))
        return gp_fail("dr_gplan_step: workspace must be 8-byte aligned");
    const int H = cfg->horizon;
    const size_t need = gp_workspace_bytes(n, H);
    if (workspace_bytes < need)
        return gp_fail("dr_gplan_step: workspace_bytes is " + std::to_string(workspace_bytes) +
                       ", needs " + std::to_string(need) + " (dr_gplan_workspace_bytes)");
    GpArgs a{};
    a.n = n;
    a.H = H;
    a.I = cfg->iterations;
    a.lr = cfg->lr;
    a.b1 = cfg->beta1;
    a.b2 = cfg->beta2;
    a.omb1 = 1.0 - cfg->beta1;
    a.omb2 = 1.0 - cfg->beta2;
    a.eps = cfg->adam_eps;
    a.w_pos = cfg->w_pos;
    a.w_vel = cfg->w_vel;
    a.w_att = cfg->w_att;
    a.w_rate = cfg->w_rate;
    a.w_eff = cfg->w_effort;
    a.w_pf = cfg->w_pos_final;
    a.w_vf = cfg->w_vel_final;
    a.obs = obs;
    a.dones = dones;
    a.nominal = nominal;
    a.m = static_cast<double *>(workspace);
    a.s = a.m + (size_t)4 * H * n;
    a.tape = a.s + (size_t)4 * H * n;
    a.U = reinterpret_cast<float *>(a.tape + (size_t)kGpTape * (H - 1) * n);
    a.actions = actions_out;
    a.cost = cost_out;
    a.grad = grad_out;
    // beta^it as the running product: one f64 rounding per iteration
    double p1 = 1.0, p2 = 1.0;
    for (int it = 0; it < a.I; ++it) {
        p1 = p1 * cfg->beta1;
        p2 = p2 * cfg->beta2;
        a.pw1[it] = p1;
        a.pw2[it] = p2;
    }
    hipLaunchKernelGGL(gplan_step_kernel, dim3((unsigned)((n + kGpBlock - 1) / kGpBlock)),
                       dim3(kGpBlock), 0, as_stream(stream), a);
    return launched(nullptr, "dr_gplan_step");
}

}  // extern "C"
