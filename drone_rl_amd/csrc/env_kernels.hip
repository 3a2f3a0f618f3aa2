// Batched quadrotor environment for MI355X (gfx950).
//
// One HIP thread owns one env for the whole step: the state lives in HBM as a
// struct of arrays (15 arrays of N: pos xyz, vel xyz, euler xyz, omega xyz,
// target xyz, then step / ep_num / eps / monitor counters), so every state
// load and store of a wave is one contiguous 512 B (f64) or 256 B (f32)
// transaction.  Actions arrive as (N,4) f32 (one 16 B load per lane).  The
// (N,15) f32 observation rows (60 B, not 16 B aligned per env) are staged
// through LDS and leave the block as contiguous float4 stores.  The moving
// variant adds 9 f32 motion arrays and 3 obs floats, the smooth variant 4 f32
// motor-force arrays and 4 obs floats (DESIGN.md sections 11 and 14).  The tag
// variant couples env 2j with env 2j+1 through in-register lane exchanges; its
// obs has 19 floats and it keeps no state of its own.
// The rk4 variant keeps a unit quaternion in place of the Euler angles (its
// fourth word is one more array of S) and advances the state by one RK4 step;
// its obs has 16 floats.  A gym handle with wind
// enabled (dr_set_wind) adds 6 f32 arrays, the mean wind and the gust, and no
// obs float.  A gym handle on waypoint courses
// (dr_set_waypoints) adds 2 i32 arrays, the waypoint's index and the reach
// counter, and moves its target on when it is reached.
// A gym handle with airframe randomisation (dr_set_airframe) adds 6 f32
// arrays, the episode's mass scale, inertia scale and motor gains, and no obs
// float.
//
// Physics: the reference's op order, restated from
//   DroneEnv.step            /root/reference/drone.py:81-159
//   DroneEnv._rotation_matrix /root/reference/drone.py:161-174 (column 2 only)
//   DroneEnv._euler_angle_rates /root/reference/drone.py:176-186
//   DroneEnv.reset           /root/reference/drone.py:48-75
//   DroneEnv._get_obs        /root/reference/drone.py:77-79
//   VectorizedDroneEnv.*     /root/reference/vectorized_drone.py:38-216
// compiled with -ffp-contract=off so no product/sum pair is fused into an FMA
// that numpy would round twice.  The state scalar S is double (reference
// precision) or float (throughput mode).

#include <cstdlib>
#include <cstring>
#include <hip/hip_ext.h>
#include <new>
#include <string>
#include <type_traits>

#include "common.h"
#include "trig.h"

#pragma clang fp contract(off)

namespace dr {
namespace {

// Physical constants (drone.py:14-43, 263; vectorized_drone.py:13-33).
constexpr double kG = 9.81;
constexpr double kMass = 1.0;
constexpr double kIxx = 0.005, kIyy = 0.005, kIzz = 0.01;
constexpr double kArm = 0.5;
constexpr double kFactor = kArm / 1.4142135623730951;  // L / np.sqrt(2)
constexpr float kKyaw32 = 0.01f;  // python float * np.float32 -> f32 (NEP 50)
constexpr double kDt = 0.02;

// DR_STAMPS (diagnostic builds only): per-wave s_memrealtime / s_memtime
// stamps at phase boundaries of env_step_kernel into a module-scope array,
// read back by dr_diag_stamps (scripts/micro/stamps.py).  Never set in the
// product build; no output element is computed from a stamp.
#ifndef DR_STAMPS
#define DR_STAMPS 0
#endif
#if DR_STAMPS
__device__ unsigned long long g_stamps[16384 * 8];
#define DR_STAMP(k)                                                            \
    do {                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                     \
        const unsigned long long t__ = __builtin_amdgcn_s_memrealtime();       \
        const unsigned w__ = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);   \
        const unsigned long long m__ = __ballot(1);                          \
        if ((int)(threadIdx.x & 63) == __ffsll((long long)m__) - 1 && w__ < 16384) \
            g_stamps[w__ * 8 + (k)] = t__;                                     \
        __builtin_amdgcn_sched_barrier(0);                                     \
    } while (0)
#else
#define DR_STAMP(k) \
    do {            \
    } while (0)
#endif
// waves per workgroup of env_step_kernel (1, 2 and 8 were measured against
// it: docs/HISTORY.md)
constexpr int kEnvWpb = 4;
constexpr int kEnvBlock = 64 * kEnvWpb;
// steps per group of the rollout kernels' next-reset Philox draw-ahead
constexpr int kResetAhead = 8;

// State loads: nontemporal (NTL) only in the large-batch launch form, where
// they measured faster; at 131,072 envs they measured 28 % slower.
template <bool NTL, typename T>
__device__ inline T ld_in(const T *p) {
    if constexpr (NTL) return __builtin_nontemporal_load(p);
    else return *p;
}
// Per-step outputs and state are written with nontemporal stores.  They
// stream to HBM while the kernel runs instead of sitting dirty in L2 until
// the end-of-kernel writeback (4-9 % faster from 65,536 to 4M envs).
template <typename T>
__device__ inline void st_out(T *p, T x) {
    store_nt(p, x);
}
// N of the Euler angles at once: the fast path runs unconditionally for
// all N (independent chains interleave; the polynomial constants are
// materialised once), the library path only for out-of-range lanes.  Each
// angle's result depends on that angle alone.
template <int N, typename S>
__device__ inline void m_sincos_n(const S *x, S *s, S *c) {
    if constexpr (sizeof(S) == 8) {
        // trig.h: 3-FMA reduction + shared polynomials (<= 1 ulp); the
        // library sincos only for |x| >= 2^19 rad, inf and NaN (a branch no
        // lane usually takes)
        int fast = 1;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const SinCos t = sincos_medium(x[k]);
            s[k] = t.s;
            c[k] = t.c;
            fast &= (int)sincos_fast_range(x[k]);
        }
        if (!fast) {
#pragma unroll
            for (int k = 0; k < N; ++k)
                if (!sincos_fast_range(x[k])) sincos(x[k], &s[k], &c[k]);
        }
    } else {
        // f32 state mode: trig.h's sincosf_medium (f64 reduction, f32
        // polynomials, <= 2 ulp); the library sincosf only out of range
        int fast = 1;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const SinCosF t = sincosf_medium(x[k]);
            s[k] = t.s;
            c[k] = t.c;
            fast &= (int)sincosf_fast_range(x[k]);
        }
        if (!fast) {
#pragma unroll
            for (int k = 0; k < N; ++k)
                if (!sincosf_fast_range(x[k])) sincosf(x[k], &s[k], &c[k]);
        }
    }
}
template <typename S>
__device__ inline void m_sincos3(const S x[3], S s[3], S c[3]) {
    m_sincos_n<3>(x, s, c);
}
__device__ inline double m_sqrt(double x) { return sqrt(x); }
__device__ inline float m_sqrt(float x) { return sqrtf(x); }

__device__ inline double m_fma(double a, double b, double c) { return fma(a, b, c); }
__device__ inline float m_fma(float a, float b, float c) { return fmaf(a, b, c); }

// x / d given rd = RN(1/d): q = RN(x*rd), then one Markstein correction with
// the exact FMA remainder, giving the correctly rounded quotient (up to
// rare 1-ulp cases) in 3 instructions instead of the ~10 of an IEEE divide.
template <typename S>
__device__ inline S div_rcp(S x, S d, S rd) {
    const S q = x * rd;
    const S r = m_fma(-q, d, x);
    return m_fma(r, rd, q);
}

enum : int { F_POS = 0, F_VEL = 3, F_EUL = 6, F_OMG = 9, F_TGT = 12, F_N = 15 };

template <typename S>
struct EnvView {
    S *f;             // F_N arrays, array k at f + k * stride
    int64_t stride;
    int32_t *step;
    int32_t *ep_num;
    double *eps;
    float *ep_ret;
    int32_t *ep_len;
    float *mot;       // moving variant: 9 f32 arrays (a xyz, w xyz, ph xyz);
                      // smooth variant: 4 f32 arrays (the motor forces)
    int64_t n;
    int64_t env_id_offset;
    const double *host_u;  // DR_RNG_HOST_UNIFORMS buffer, else nullptr
    uint32_t seed_lo, seed_hi;
    int32_t max_steps;
    S dt;
    __host__ __device__ S *field(int k) const { return f + k * stride; }
};

// Byte offsets of the per-env arrays inside a handle's one allocation of
// `sp` (stride) elements per array: F_N state arrays of S, then eps (f64),
// step, ep_num (i32), the VecMonitor return (f32) and length (i32), then the
// moving variant's 9 f32 motion arrays.  Shared by view_of and the step
// kernel, which forms its array bases from (f, stride) in scalar registers.
template <typename S>
struct Layout {
    __host__ __device__ static int64_t eps(int64_t sp) { return (int64_t)F_N * sp * sizeof(S); }
    __host__ __device__ static int64_t step(int64_t sp) { return eps(sp) + sp * 8; }
    __host__ __device__ static int64_t ep_num(int64_t sp) { return step(sp) + sp * 4; }
    __host__ __device__ static int64_t ep_ret(int64_t sp) { return ep_num(sp) + sp * 4; }
    __host__ __device__ static int64_t ep_len(int64_t sp) { return ep_ret(sp) + sp * 4; }
    __host__ __device__ static int64_t mot(int64_t sp) { return ep_len(sp) + sp * 4; }
};

// The step kernel's per-field base pointers (f + k * stride), passed as
// separate uniform kernel arguments so each SoA access is an SGPR base plus
// one shared 32-bit lane offset (the compiler folds f + k*stride + i*8 into
// per-field 64-bit VGPR address arithmetic otherwise).  Kernel-argument
// preloading into SGPRs (gfx950) was measured as the alternative: slower by
// 0.1 us at 65,536 envs (the scalar address chain it needs costs more than
// the one scalar-load round trip it saves).
template <typename S>
struct FieldPtrs {
    S *p[F_N];
    int32_t *step, *ep_num;
    double *eps;
};

struct StepIO {
    const float *actions;
    float *obs;
    float *rew;
    uint8_t *done;
    float *term_obs;
    float *ep_ret_out;
    int32_t *ep_len_out;
    int auto_reset;
    // MON only, nullable: 1 where the episode ended at the step limit
    // without a crash (the gymnasium TimeLimit "truncated" flag)
    uint8_t *trunc_out;
};

// The five reset draws of env i starting episode `ep_new`, in the reference
// order: pos x, pos y, target x, y, z (drone.py:57,73).  mode: 0 Philox,
// 1 host buffer, 2 constant 0.5 (constructor reset in host-uniform mode).
// NU = 5 (gym) or 14 (moving: the 5 gym draws, then 9 motion draws; the
// first 5 are the gym variant's, so eps = 0 reproduces it exactly).
template <int NU, typename S>
__device__ inline void reset_uniforms(const EnvView<S> &v, int64_t i,
                                      int32_t ep_new, int mode, double u[NU],
                                      const u32x4 *pre = nullptr) {
    if (mode == 1) {
#pragma unroll
        for (int k = 0; k < NU; ++k) u[k] = v.host_u[i * NU + k];
        return;
    }
    if (mode == 2) {
#pragma unroll
        for (int k = 0; k < NU; ++k) u[k] = 0.5;
        return;
    }
    const uint64_t gid = (uint64_t)(v.env_id_offset + i);
#pragma unroll
    for (int b = 0; b < (NU + 3) / 4; ++b) {
        // pre: the blocks already drawn for this (episode, env)
        const u32x4 r = pre ? pre[b]
                            : philox4x32_10(u32x4{(uint32_t)ep_new, (uint32_t)gid,
                                                  (uint32_t)(gid >> 32), TAG_RESET | (uint32_t)b},
                                            v.seed_lo, v.seed_hi);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * b + k < NU) u[4 * b + k] = u01_w32(w[k]);
    }
}

// DroneEnv.reset (drone.py:48-75) on registers st[F_N]; updates ep_num/eps
// in memory, returns the new step counter (0).
template <typename S>
__device__ inline void gym_reset_regs(const EnvView<S> &v, int64_t i, int mode,
                                      S st[F_N], int32_t ep_old, double eps,
                                      const u32x4 *pre0 = nullptr) {
    const int32_t ep_new = ep_old + 1;        // ep_num += 1          (61)
    if (ep_new % 2000 == 0) {                 // curriculum bump      (68-70)
        eps += 0.1;
        v.eps[i] = eps;
    }
    double u[5];
    if (mode == 0) {
        // Philox block 0 = (pos x, pos y, target x, target y); block 1 word
        // 0 = target z.  The target draws are multiplied by eps, and 0 * u
        // is exactly +0 for the uniforms in [0,1): while the curriculum is
        // at eps == 0 (the first 2000 episodes of every env) block 1 cannot
        // change any result bit, so it is skipped.
        const uint64_t gid = (uint64_t)(v.env_id_offset + i);
        const u32x4 r0 = pre0 ? *pre0
                              : philox4x32_10(u32x4{(uint32_t)ep_new, (uint32_t)gid,
                                                    (uint32_t)(gid >> 32), TAG_RESET},
                                              v.seed_lo, v.seed_hi);
        u[0] = u01_w32(r0.x);
        u[1] = u01_w32(r0.y);
        u[2] = u01_w32(r0.z);
        u[3] = u01_w32(r0.w);
        u[4] = 0.0;
        if (eps != 0.0) {
            const u32x4 r1 = philox4x32_10(
                u32x4{(uint32_t)ep_new, (uint32_t)gid, (uint32_t)(gid >> 32), TAG_RESET | 1u},
                v.seed_lo, v.seed_hi);
            u[4] = u01_w32(r1.x);
        }
    } else {
        reset_uniforms<5>(v, i, ep_new, mode, u);
    }
    DR_STAMP(6);
    v.ep_num[i] = ep_new;
    st[F_POS + 0] = (S)(u[0] - 0.5);          // (57)
    st[F_POS + 1] = (S)(u[1] - 0.5);
    st[F_POS + 2] = (S)1.0;
#pragma unroll
    for (int k = 3; k < 12; ++k) st[k] = (S)0;   // vel, euler, omega (58-60)
    st[F_TGT + 0] = (S)(eps * u[2]);          // (73)
    st[F_TGT + 1] = (S)(eps * u[3]);
    st[F_TGT + 2] = (S)(eps * u[4] + 1.0 + 0.0);
    DR_STAMP(7);
}

// The state DroneEnv.reset would start episode ep_old + 1 from (drone.py:
// 48-75), formed from that episode's first Philox block r0 exactly as
// gym_reset_regs forms it (the curriculum bump, then the draws, the same
// expressions), so that a reset inside the split-physics rollout kernel is a
// register copy of state prepared when the block was drawn, off the step in
// which some lane of the wave resets (round 5).
template <typename S>
struct GymNext {
    S px, py, tx, ty, tz;
    double eps;               // eps after episode ep_old + 1's curriculum bump
    bool bump;                // ep_old + 1 bumps the curriculum
};
template <typename S>
__device__ inline GymNext<S> gym_next_reset(const EnvView<S> &v, uint64_t gid, int32_t ep_old,
                                            double eps, const u32x4 &r0) {
    const int32_t ep_new = ep_old + 1;
    GymNext<S> g;
    g.bump = ep_new % 2000 == 0;
    if (g.bump) eps += 0.1;
    double u4 = 0.0;
    if (eps != 0.0) {
        const u32x4 r1 = philox4x32_10(
            u32x4{(uint32_t)ep_new, (uint32_t)gid, (uint32_t)(gid >> 32), TAG_RESET | 1u},
            v.seed_lo, v.seed_hi);
        u4 = u01_w32(r1.x);
    }
    g.px = (S)(u01_w32(r0.x) - 0.5);
    g.py = (S)(u01_w32(r0.y) - 0.5);
    g.tx = (S)(eps * u01_w32(r0.z));
    g.ty = (S)(eps * u01_w32(r0.w));
    g.tz = (S)(eps * u4 + 1.0 + 0.0);
    g.eps = eps;
    return g;
}

template <typename S>
__device__ inline void vec_reset_regs(S st[F_N]) {
    // VectorizedDroneEnv.reset: every env at (0.1,0.1,0.1), at rest
    // (vectorized_drone.py:50-53); fixed target (0,0,10) (line 30).
#pragma unroll
    for (int k = 0; k < 3; ++k) st[F_POS + k] = (S)0.1;
#pragma unroll
    for (int k = 3; k < 12; ++k) st[k] = (S)0;
    st[F_TGT + 0] = (S)0;
    st[F_TGT + 1] = (S)0;
    st[F_TGT + 2] = (S)10.0;
}

// ---- moving-target variant (DR_VARIANT_MOVING) ----
// target_k(s) = c_k + a_k sin(w_k s dt + ph_k), velocity a_k w_k cos(...),
// evaluated in f32 (the motion is this build's spec, not the reference's).
template <typename S>
__device__ inline void moving_target(const S c[3], const float mp[9], int32_t s,
                                     float dt, S tgt[3], float tvel[3]) {
    const float t = (float)s * dt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float sn, cs;
        sincosf(mp[3 + k] * t + mp[6 + k], &sn, &cs);
        tgt[k] = c[k] + (S)(mp[k] * sn);
        tvel[k] = mp[k] * mp[3 + k] * cs;
    }
}

// DroneEnv.reset plus the motion draws: pos / zeroed rates / centre exactly
// as gym_reset_regs (centre = the gym target), a = eps * U, w = 0.5 + 1.5 U
// rad/s, ph = 2 pi U.
template <typename S>
__device__ inline void moving_reset_regs(const EnvView<S> &v, int64_t i, int mode,
                                         S st[F_N], S c[3], float mp[9],
                                         int32_t ep_old, double eps,
                                         const u32x4 *pre4 = nullptr) {
    const int32_t ep_new = ep_old + 1;
    double u[14];
    reset_uniforms<14>(v, i, ep_new, mode, u, pre4);
    if (ep_new % 2000 == 0) {
        eps += 0.1;
        v.eps[i] = eps;
    }
    v.ep_num[i] = ep_new;
    st[F_POS + 0] = (S)(u[0] - 0.5);
    st[F_POS + 1] = (S)(u[1] - 0.5);
    st[F_POS + 2] = (S)1.0;
#pragma unroll
    for (int k = 3; k < 12; ++k) st[k] = (S)0;
    c[0] = (S)(eps * u[2]);
    c[1] = (S)(eps * u[3]);
    c[2] = (S)(eps * u[4] + 1.0 + 0.0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mp[k] = (float)(eps * u[5 + k]);
        mp[3 + k] = (float)(0.5 + 1.5 * u[8 + k]);
        mp[6 + k] = (float)(6.283185307179586 * u[11 + k]);
    }
}

// The gym variant with wind enabled (dr_set_wind): a
// kernel-variant tag of this file, not a public dr_variant value.  A gym
// handle's kernels are instantiated on it once its wind arrays exist.
constexpr int KVAR_WIND = 64;
// The gym variant with waypoint courses enabled (dr_set_waypoints; DESIGN.md
// section 18): likewise a tag of this file.  Wind and waypoints exclude each
// other on a handle.
constexpr int KVAR_WAYPOINT = 65;
// The gym variant with per-episode airframe randomisation enabled
// (dr_set_airframe): likewise a tag of this file.  The
// three options exclude each other pairwise on a handle.
constexpr int KVAR_AIRFRAME = 66;

// What the kernels and the host ask about a variant, in one place (DESIGN.md
// section 20).  One line per variant:
//   vectorized  no stored target, no per-env reset, 12 obs floats
//   gym         the reference env: stored target, curriculum reset
//   moving      the gym's reset plus a target on a Lissajous path: centre and
//               9 motion words beside the state, 3 more obs floats
//   smooth      the gym env behind a motor lag: 4 force words, 4 obs floats
//   tag         gym drones in pairs; the gym's target carried unread, 7 obs
//               floats past the first 12 from the partner, no words of its own
//   rk4         the gym's task on a quaternion state and an RK4 step: one
//               more word of S, 1 more obs float
//   wind        the gym's step behind a disturbance: 6 words, no obs float
//   waypoint    the gym's step, a target that moves on when reached: 2 words
//   airframe    the gym's step on the episode's mass, inertia and motor
//               gains: 6 words
template <int VAR>
struct Traits {
    static constexpr bool VEC = VAR == DR_VARIANT_VECTORIZED;
    static constexpr bool MOVING = VAR == DR_VARIANT_MOVING;
    static constexpr bool SMOOTH = VAR == DR_VARIANT_SMOOTH;
    static constexpr bool TAG = VAR == DR_VARIANT_TAG;
    static constexpr bool RK4 = VAR == DR_VARIANT_RK4;
    static constexpr bool WIND = VAR == KVAR_WIND;
    static constexpr bool WAYPT = VAR == KVAR_WAYPOINT;
    static constexpr bool AIRF = VAR == KVAR_AIRFRAME;
    // a gym handle with one of its options enabled
    static constexpr bool OPTION = WIND || WAYPT || AIRF;
    // per-env episodes, curriculum and reset draws
    static constexpr bool GYMLIKE = !VEC;
    // the gym's stored target and reset
    static constexpr bool GYMSTATE = GYMLIKE && !MOVING;
    // observation width
    static constexpr int OD = MOVING ? 18 : (SMOOTH || TAG) ? 19 : RK4 ? 16 : VEC ? 12 : 15;
    // Philox blocks per reset
    static constexpr int NB = MOVING ? 4 : 1;
    // carries side words in a Side (below); moving's, smooth's and wind's
    // are locals of the kernels
    static constexpr bool SIDE = RK4 || WAYPT || AIRF;
    // its side state's reset is a pure draw, made ahead with the reset's blocks
    static constexpr bool SIDE_AHEAD = AIRF;
    // host: the rollout has the one-role kernel only (the side state and the
    // partner exchange are not built into the warp-specialised forms)
    static constexpr bool ONE_ROLE = SMOOTH || TAG || RK4 || OPTION;
    // host: an option resets as the gym does, then refills its words
    static constexpr int RESET_VAR = OPTION ? (int)DR_VARIANT_GYM : VAR;
    // host: bytes per env behind the monitor counters (Layout::mot)
    template <typename S>
    static constexpr size_t mot_bytes() {
        return MOVING ? 9 * sizeof(float) : SMOOTH ? 4 * sizeof(float) : RK4 ? sizeof(S) : 0;
    }
};

// ---- smooth-control variant (DR_VARIANT_SMOOTH) ----
// What a variant's kernels take beyond the shared arguments: nothing, or the
// smooth / tag variant's two parameters.  A trailing kernel argument of its own, so
// the argument blocks of the other variants' kernels stay as they were.
template <int VAR>
struct VarArgs {};
template <>
struct VarArgs<DR_VARIANT_SMOOTH> {
    float alpha;   // lag blend dt / (tau + dt), in (0, 1]
    float lam;     // action-rate penalty, >= 0
};
template <>
struct VarArgs<DR_VARIANT_TAG> {
    float radius;  // tag radius R > 0
    float crash;   // crash penalty c >= 0
};
template <>
struct VarArgs<DR_VARIANT_RK4> {
    // dt / 6 formed on the host in the state scalar (one IEEE divide per
    // handle instead of one per lane and step): f64 and f32 state
    double h6d;
    float h6f;
};
// the force every motor applies after a reset: f32(mass * g / 4)
constexpr float kHover32 = (float)(kMass * kG / 4);

// The motor lag on registers: f <- (1 - alpha) f + alpha a, every operation
// one f32 rounding (no FMA: the file is compiled with contraction off).
// Returns the forces as the action the physics sees and sets dev_sq = |a - f|^2
// against the forces BEFORE the update.
__device__ inline float4 smooth_filter(float4 a, float f[4], float alpha, float &dev_sq) {
    const float c[4] = {a.x, a.y, a.z, a.w};
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = c[j] - f[j];
    dev_sq = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3];
    const float b = 1.0f - alpha;
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = b * f[j] + alpha * c[j];
    return make_float4(f[0], f[1], f[2], f[3]);
}

// ---- wind, gusts and linear drag (dr_set_wind) ----
// Per env six f32 words, the episode's mean wind m and the gust g, in six
// arrays at EnvView::mot (the handle's second allocation, same stride).
template <>
struct VarArgs<KVAR_WIND> {
    float k;   // linear drag per unit mass, 1/s
    float b;   // gust persistence 1 - gust_rate
    float c;   // gust noise scale sigma sqrt(3 (1 - b^2)), formed on the host
    float W;   // bound of each axis of the mean wind; read by resets only
};
// f32(2u - 1) of a Philox word's 32-bit uniform: the subtraction is exact in
// f64, the cast is the one rounding.
__device__ inline float wind_pm1(uint32_t w) { return (float)(2.0 * u01_w32(w) - 1.0); }

// The mean wind of env `gid` in episode `ep`: the reset stream's block 2.
__device__ inline void wind_mean(uint32_t k0, uint32_t k1, uint64_t gid, int32_t ep, float W,
                                 float m[3]) {
    const u32x4 r = philox4x32_10(
        u32x4{(uint32_t)ep, (uint32_t)gid, (uint32_t)(gid >> 32), TAG_RESET | 2u}, k0, k1);
    m[0] = W * wind_pm1(r.x);
    m[1] = W * wind_pm1(r.y);
    m[2] = W * wind_pm1(r.z);
}

// The disturbance ahead of the gym step of an env at step counter `s` of
// episode `ep`: the gust's AR(1) update, every operation one f32 rounding,
// then the drag impulse on the velocity towards the air's, in S.  Always
// drawn: at c == 0 the product c * xi is a zero whose sign is xi's.
template <typename S>
__device__ inline void wind_pre(S st[F_N], const float m[3], float g[3],
                                const VarArgs<KVAR_WIND> &va, uint32_t k0, uint32_t k1,
                                uint64_t gid, int32_t ep, int32_t s, S dt) {
    const u32x4 r = philox4x32_10(
        u32x4{(uint32_t)ep, (uint32_t)gid, (uint32_t)(gid >> 32), TAG_GUST | (uint32_t)s}, k0, k1);
    const float xi[3] = {wind_pm1(r.x), wind_pm1(r.y), wind_pm1(r.z)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[k] = va.b * g[k] + va.c * xi[k];
        const S w = (S)(m[k] + g[k]);
        st[F_VEL + k] = st[F_VEL + k] + ((S)va.k * (w - st[F_VEL + k])) * dt;
    }
}

// ---- waypoint courses (dr_set_waypoints) ----
// Per env two i32 words, the index j of the current waypoint within the
// episode and the count q of reaches since enabling, in two arrays at
// EnvView::mot (the handle's second allocation, same stride).  The current
// waypoint is the gym's stored target.
template <>
struct VarArgs<KVAR_WAYPOINT> {
    float radius;  // reach radius R > 0
    float bonus;   // reach bonus B >= 0
};

// Waypoint number `j` (>= 1) of env `gid` in episode `ep`, into st[F_TGT ..]:
// the expressions of gym_reset_regs on a Philox block of its own.  While
// eps == 0 the products are exact zeros, the waypoint is (0, 0, 1) and the draw
// is skipped.  Called inside the divergent `reached` branch only: a reach is a
// rare event, and the ten rounds stay off the step's straight-line path.
template <typename S>
__device__ inline void waypoint_draw(S st[F_N], uint32_t k0, uint32_t k1, uint64_t gid,
                                     int32_t ep, double eps, int32_t j) {
    double u[3] = {0.0, 0.0, 0.0};
    if (eps != 0.0) {
        const u32x4 r = philox4x32_10(u32x4{(uint32_t)ep, (uint32_t)gid, (uint32_t)(gid >> 32),
                                            TAG_WAYPOINT | (uint32_t)j},
                                      k0, k1);
        u[0] = u01_w32(r.x);
        u[1] = u01_w32(r.y);
        u[2] = u01_w32(r.z);
    }
    st[F_TGT + 0] = (S)(eps * u[0]);
    st[F_TGT + 1] = (S)(eps * u[1]);
    st[F_TGT + 2] = (S)(eps * u[2] + 1.0 + 0.0);
}

// ---- airframe randomisation (dr_set_airframe) ----
// Per env six f32 words, the episode's mass scale m, inertia scale s and
// motor gains g0..g3, in six arrays at EnvView::mot (the handle's second
// allocation, same stride).  Resets are their only writers.
template <>
struct VarArgs<KVAR_AIRFRAME> {
    float sm;   // spread of the mass scale; the three are read by resets only
    float si;   // spread of the inertia scale
    float sg;   // spread of each motor gain
};

// The airframe of env `gid` in episode `ep`: af = (m, s, g0..g3), each
// 1.0f + spread * xi in f32 (a product, a sum).  At spread 0 the value is
// exactly 1.0f for every xi, so a block whose spreads are 0 is skipped.
__device__ inline void airframe_draw(uint32_t k0, uint32_t k1, uint64_t gid, int32_t ep,
                                     const VarArgs<KVAR_AIRFRAME> &va, float af[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) af[k] = 1.0f;
    if (va.sm != 0.f || va.si != 0.f) {
        const u32x4 r = philox4x32_10(
            u32x4{(uint32_t)ep, (uint32_t)gid, (uint32_t)(gid >> 32), TAG_AIRFRAME | 0u}, k0, k1);
        af[0] = 1.0f + va.sm * wind_pm1(r.x);
        af[1] = 1.0f + va.si * wind_pm1(r.y);
    }
    if (va.sg != 0.f) {
        const u32x4 r = philox4x32_10(
            u32x4{(uint32_t)ep, (uint32_t)gid, (uint32_t)(gid >> 32), TAG_AIRFRAME | 1u}, k0, k1);
        af[2] = 1.0f + va.sg * wind_pm1(r.x);
        af[3] = 1.0f + va.sg * wind_pm1(r.y);
        af[4] = 1.0f + va.sg * wind_pm1(r.z);
        af[5] = 1.0f + va.sg * wind_pm1(r.w);
    }
}

// An env's airframe in registers: the six words and the reciprocals of the
// two scales, IEEE f32 divides formed when the words are loaded or drawn, not
// per step.
struct Airframe {
    float w[6];   // m, s, g0..g3
    float im, is;
    __device__ void recip() {
        im = 1.0f / w[0];
        is = 1.0f / w[1];
    }
};
// a'_j = g_j a_j, the command the motor mixes are taken on
__device__ inline float4 airframe_gain(const Airframe &a, float4 act) {
    return make_float4(a.w[2] * act.x, a.w[3] * act.y, a.w[4] * act.z, a.w[5] * act.w);
}

// ---- tag variant (DR_VARIANT_TAG) ----
// Envs 2j (pursuer) and 2j+1 (evader) sit in lanes l and l^1 of one wave.
// The partner's value of a register: a lane <-> lane^1 swap that touches no
// memory.  It must execute with all 64 lanes of the wave active (a lane
// reads what its partner holds, and an inactive partner supplies nothing),
// so it is only ever called from wave-uniform code.
// DPP quad_perm:[1,0,3,2], one v_mov_b32_dpp per dword (__shfl_xor(., 1), a
// ds_bpermute_b32 per dword, measured slower: DESIGN.md section 15).
__device__ inline int partner_of(int x) {
    // quad_perm [1,0,3,2] = 1 | 0 << 2 | 3 << 4 | 2 << 6
    return __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false);
}
__device__ inline float partner_of(float x) {
    return __int_as_float(partner_of(__float_as_int(x)));
}
__device__ inline double partner_of(double x) {
    return __hiloint2double(partner_of(__double2hiint(x)), partner_of(__double2loint(x)));
}
// The partner's position and velocity (6 x S).
template <typename S>
__device__ inline void tag_partner(const S st[F_N], S pp[3], S pv[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pp[k] = partner_of(st[F_POS + k]);
        pv[k] = partner_of(st[F_VEL + k]);
    }
}
// The obs past the gym's first 12: partner - own position and velocity
// (S subtract, then the cast, as the gym's target - pos), then the role.
template <typename S>
__device__ inline void tag_ext(const S st[F_N], const S pp[3], const S pv[3], float sigma,
                               float ext[7]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ext[k] = (float)(pp[k] - st[F_POS + k]);
        ext[3 + k] = (float)(pv[k] - st[F_VEL + k]);
    }
    ext[6] = sigma;
}
// The pursuer's reward g = 0.01 * (-d) [+ 1 inside R], the evader's -g, on
// the new positions.  d is the same bit for bit in both lanes: the
// differences are negatives of each other and the squares equal.
template <typename S>
__device__ inline S tag_reward(const S st[F_N], const S pp[3], float radius, bool pursuer) {
    const S dx = st[F_POS + 0] - pp[0];
    const S dy = st[F_POS + 1] - pp[1];
    const S dz = st[F_POS + 2] - pp[2];
    const S d = m_sqrt((dx * dx + dy * dy) + dz * dz);
    S g = (S)0.01 * -d;
    if (d < (S)radius) g += (S)1;
    return pursuer ? g : -g;
}

// `ext`: the floats past the gym's 15 (moving: the target velocity, 3;
// smooth: the motor forces, 4); tag: the 7 floats past the first 12
// (tag_ext).
template <typename S, int VAR>
__device__ inline void make_obs(const S st[F_N], float ob[Traits<VAR>::OD],
                                const float *ext = nullptr) {
    using T = Traits<VAR>;
    if constexpr (T::RK4) {
        // p, v, q = (a, b, c, d), omega, target - p; ext[0] = f32(d)
#pragma unroll
        for (int k = 0; k < 9; ++k) ob[k] = (float)st[k];
        ob[9] = ext[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) ob[10 + k] = (float)st[F_OMG + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) ob[13 + k] = (float)(st[F_TGT + k] - st[F_POS + k]);
        return;
    }
    // _get_obs: f32(concat(pos, vel, euler, omega[, target - pos]))  (79)
#pragma unroll
    for (int k = 0; k < 12; ++k) ob[k] = (float)st[k];
    if constexpr (T::TAG) {
#pragma unroll
        for (int k = 0; k < 7; ++k) ob[12 + k] = ext[k];
    } else if constexpr (!T::VEC) {
#pragma unroll
        for (int k = 0; k < 3; ++k) ob[12 + k] = (float)(st[F_TGT + k] - st[F_POS + k]);
    }
    if constexpr (T::MOVING) {
#pragma unroll
        for (int k = 0; k < 3; ++k) ob[15 + k] = ext[k];
    }
    if constexpr (T::SMOOTH) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ob[15 + k] = ext[k];
    }
}

// One physics step on registers.  Returns the reward, sets `crash` (z<0 or
// |p|>50).  VAR selects the two places the variants differ (W row 3 and the
// reward form / bonus radius).
// The action's motor mixes (drone.py:106, 113-117): total thrust and the
// three torques' f32 sums, before any state is involved.
struct MotorMix {
    float thr, phi, theta, psi;
};
__device__ inline MotorMix motor_mix(float4 act) {
    const float a0 = act.x, a1 = act.y, a2 = act.z, a3 = act.w;
    return MotorMix{((a0 + a1) + a2) + a3, ((a0 + a1) - a2) - a3,
                    ((-a0 + a1) + a2) - a3, ((a0 - a1) + a2) - a3};
}

// wp / reached: the waypoint option's radius and bonus and its reach flag
// (KVAR_WAYPOINT only).  af: the env's airframe (KVAR_AIRFRAME only: no other
// instantiation forms or reads one).
template <typename S, int VAR>
__device__ inline S physics_step_mixed(S st[F_N], MotorMix mx, S dt, bool &crash,
                                       const VarArgs<VAR> *wp = nullptr,
                                       bool *reached = nullptr,
                                       const Airframe *af = nullptr) {
    using TR = Traits<VAR>;
    // thrust / torques (drone.py:106, 113-117): f32 sums, f64 factor product,
    // the yaw torque stays f32.
    const float thr = mx.thr;
    S tau_phi = (S)kFactor * (S)mx.phi;
    S tau_theta = (S)kFactor * (S)mx.theta;
    const float tau_psi = kKyaw32 * mx.psi;
    if constexpr (TR::AIRF) {
        // inertia s (Ixx, Iyy, Izz): one common scale leaves the gyroscopic
        // terms as they are, so only the torques scale (the yaw torque below)
        tau_phi = tau_phi * (S)af->is;
        tau_theta = tau_theta * (S)af->is;
    }

    // One sincos per angle: a shared range reduction yields exactly the
    // separate sin() and cos() results at half the instructions.
    S sn[3], cs[3];
    m_sincos3(&st[F_EUL], sn, cs);
    DR_STAMP(1);
    const S sph = sn[0], cph = cs[0], sth = sn[1], cth = cs[1], sps = sn[2], cps = cs[2];
    // R(old euler) column 2 (drone.py:169-173): thrust is body-z only.
    const S r02 = cps * sth * cph + sps * sph;
    const S r12 = sps * sth * cph - cps * sph;
    const S r22 = cth * cph;
    const S T = (S)thr;
    S acc0, acc1, acc2;
    if constexpr (TR::AIRF) {
        // mass m kMass: the reciprocal's product where the gym divides
        acc0 = (S)0 + (r02 * T) * (S)af->im;
        acc1 = (S)0 + (r12 * T) * (S)af->im;
        acc2 = (S)(-kG) + (r22 * T) * (S)af->im;
    } else {
        acc0 = (S)0 + (r02 * T) / (S)kMass;      // (124)
        acc1 = (S)0 + (r12 * T) / (S)kMass;
        acc2 = (S)(-kG) + (r22 * T) / (S)kMass;
    }
    st[F_VEL + 0] += acc0 * dt;                      // (127)
    st[F_VEL + 1] += acc1 * dt;
    st[F_VEL + 2] += acc2 * dt;
#pragma unroll
    for (int k = 0; k < 3; ++k) st[F_POS + k] += st[F_VEL + k] * dt;  // (128)

    // Euler-angle rates from the OLD omega (131-132, 176-186).
    const S w0 = st[F_OMG + 0], w1 = st[F_OMG + 1], w2 = st[F_OMG + 2];
    // tan(theta) from the shared sincos (np.tan rounds once; this rounds the
    // quotient once more: <= 2 ulp apart, far inside the parity bar).
    const S sec = (S)1 / cth;        // the only IEEE divide; also vd:116
    const S tth = div_rcp(sth, cth, sec);
    S ed2;
    if constexpr (!TR::VEC) {
        ed2 = ((S)0 * w0 + div_rcp(sph, cth, sec) * w1) +
              div_rcp(cph, cth, sec) * w2;                             // (184)
    } else {
        ed2 = ((S)0 * w0 + (sph * sec) * w1) + (cph * sec) * w2;
    }
    const S ed0 = ((S)1 * w0 + (sph * tth) * w1) + (cph * tth) * w2;
    const S ed1 = ((S)0 * w0 + cph * w1) + (-sph) * w2;
    st[F_EUL + 0] += ed0 * dt;
    st[F_EUL + 1] += ed1 * dt;
    st[F_EUL + 2] += ed2 * dt;

    // Angular dynamics, diagonal inertia, old omega (135-139).
    const S wd0 = div_rcp(tau_phi - (S)(kIyy - kIzz) * w1 * w2, (S)kIxx, (S)(1.0 / kIxx));
    const S wd1 = div_rcp(tau_theta - (S)(kIzz - kIxx) * w0 * w2, (S)kIyy, (S)(1.0 / kIyy));
    S tau_psi_s;
    if constexpr (TR::AIRF) tau_psi_s = (S)tau_psi * (S)af->is;
    else tau_psi_s = (S)tau_psi;
    const S wd2 = div_rcp(tau_psi_s - (S)(kIxx - kIyy) * w0 * w1, (S)kIzz, (S)(1.0 / kIzz));
    st[F_OMG + 0] += wd0 * dt;
    st[F_OMG + 1] += wd1 * dt;
    st[F_OMG + 2] += wd2 * dt;

    // Reward on the new position (142-148; vectorized_drone.py:204-207).
    // The tag variant's reward needs the partner's new position: the caller
    // forms it (tag_reward) after the exchange.
    S r = (S)0;
    if constexpr (!TR::TAG) {
        const S dx = st[F_POS + 0] - st[F_TGT + 0];
        const S dy = st[F_POS + 1] - st[F_TGT + 1];
        const S dz = st[F_POS + 2] - st[F_TGT + 2];
        const S d = m_sqrt((dx * dx + dy * dy) + dz * dz);
        if constexpr (TR::WAYPT) {
            // the gym's form on the handle's radius and bonus; the caller
            // advances the course where `reached`
            r = (S)0.01 * -d;
            *reached = d < (S)wp->radius;
            if (*reached) r += (S)wp->bonus;
        } else if constexpr (!TR::VEC) {
            r = (S)0.01 * -d;
            if (d < (S)0.05) r += (S)1;
        } else {
            r = (S)(-0.01) * d;
            if (d < (S)1) r += (S)1;
        }
    }
    // Termination (154; vectorized_drone.py:211).  NaN compares false.
    const S px = st[F_POS + 0], py = st[F_POS + 1], pz = st[F_POS + 2];
    // norm(p) > 50  <=>  |p|^2 > 2500 exactly: sqrt is correctly rounded and
    // the next representable square above 2500 already rounds above 50
    // (f64 and f32 alike); NaN compares false either way.
    const S pn2 = (px * px + py * py) + pz * pz;
    crash = (pz < (S)0) || (pn2 > (S)2500);
    return r;
}

template <typename S, int VAR>
__device__ inline S physics_step(S st[F_N], float4 act, S dt, bool &crash,
                                 const VarArgs<VAR> *wp = nullptr, bool *reached = nullptr,
                                 const Airframe *af = nullptr) {
    return physics_step_mixed<S, VAR>(st, motor_mix(act), dt, crash, wp, reached, af);
}

// ---- rk4 variant (DR_VARIANT_RK4) ----
// The gym env's task on the state y = (p, v, q, omega), q = (a, b, c, d) =
// (w, x, y, z) a unit quaternion body -> world, advanced by one classic RK4
// step with the action held.  In the kernels' registers a, b, c sit where
// the Euler angles do (st[F_EUL ..]) and d in a register of its own, `qd`;
// in memory d is one more array of S behind the monitor counters
// (Layout::mot).  Every operation is one correctly rounded IEEE operation in
// the order tests/rk4_ref.py fixes; there is no trigonometric function and
// no divide but the normalisation's.
enum : int { Y_P = 0, Y_V = 3, Y_Q = 6, Y_W = 10, Y_N = 13 };

// dy/dt at y under thrust T and torques tau.
template <typename S>
__device__ inline void rk4_deriv(const S y[Y_N], S T, const S tau[3], S k[Y_N]) {
    const S rM = (S)1 / (S)kMass, rIx = (S)1 / (S)kIxx, rIy = (S)1 / (S)kIyy,
            rIz = (S)1 / (S)kIzz;
    const S a = y[Y_Q + 0], b = y[Y_Q + 1], c = y[Y_Q + 2], d = y[Y_Q + 3];
    const S w0 = y[Y_W + 0], w1 = y[Y_W + 1], w2 = y[Y_W + 2];
    // R(q) column 2: the thrust is body-z only
    const S r02 = (S)2 * (b * d + a * c);
    const S r12 = (S)2 * (c * d - a * b);
    const S r22 = (S)1 - (S)2 * (b * b + c * c);
#pragma unroll
    for (int j = 0; j < 3; ++j) k[Y_P + j] = y[Y_V + j];
    k[Y_V + 0] = (r02 * T) * rM;
    k[Y_V + 1] = (r12 * T) * rM;
    k[Y_V + 2] = (S)(-kG) + (r22 * T) * rM;
    // q' = q (x) (0, omega) / 2
    k[Y_Q + 0] = (S)0.5 * (((-b * w0) - c * w1) - d * w2);
    k[Y_Q + 1] = (S)0.5 * ((a * w0 + c * w2) - d * w1);
    k[Y_Q + 2] = (S)0.5 * ((a * w1 - b * w2) + d * w0);
    k[Y_Q + 3] = (S)0.5 * ((a * w2 + b * w1) - c * w0);
    // the gym's angular dynamics (drone.py:135-139) with the reciprocals
    k[Y_W + 0] = (tau[0] - ((S)(kIyy - kIzz) * w1) * w2) * rIx;
    k[Y_W + 1] = (tau[1] - ((S)(kIzz - kIxx) * w0) * w2) * rIy;
    k[Y_W + 2] = (tau[2] - ((S)(kIxx - kIyy) * w0) * w1) * rIz;
}

// One step on registers: st[0..8] = p, v, (a, b, c); qd = d; st[F_OMG ..] =
// omega; st[F_TGT ..] = target.  h6 = dt / 6.  Returns the gym's reward on
// the new position and sets `crash` as physics_step_mixed does.
template <typename S>
__device__ inline S rk4_step(S st[F_N], S &qd, MotorMix mx, S dt, S h6, bool &crash) {
    const S T = (S)mx.thr;
    const S tau[3] = {(S)kFactor * (S)mx.phi, (S)kFactor * (S)mx.theta,
                      (S)(kKyaw32 * mx.psi)};
    S y[Y_N], yt[Y_N], k[Y_N], s12[Y_N], s34[Y_N];
#pragma unroll
    for (int j = 0; j < 9; ++j) y[j] = st[j];
    y[Y_Q + 3] = qd;
#pragma unroll
    for (int j = 0; j < 3; ++j) y[Y_W + j] = st[F_OMG + j];
    const S h2 = dt * (S)0.5;
    rk4_deriv(y, T, tau, k);                               // k1
#pragma unroll
    for (int j = 0; j < Y_N; ++j) {
        s12[j] = k[j];
        yt[j] = y[j] + h2 * k[j];
    }
    rk4_deriv(yt, T, tau, k);                              // k2
#pragma unroll
    for (int j = 0; j < Y_N; ++j) {
        s12[j] = s12[j] + (S)2 * k[j];
        yt[j] = y[j] + h2 * k[j];
    }
    rk4_deriv(yt, T, tau, k);                              // k3
#pragma unroll
    for (int j = 0; j < Y_N; ++j) {
        s34[j] = (S)2 * k[j];
        yt[j] = y[j] + dt * k[j];
    }
    rk4_deriv(yt, T, tau, k);                              // k4
#pragma unroll
    for (int j = 0; j < Y_N; ++j) y[j] = y[j] + h6 * (s12[j] + (s34[j] + k[j]));
    // back onto the unit sphere: an IEEE sqrt and divide
    const S qa = y[Y_Q + 0], qb = y[Y_Q + 1], qc = y[Y_Q + 2], qq = y[Y_Q + 3];
    const S n2 = ((qa * qa + qb * qb) + qc * qc) + qq * qq;
    const S rn = (S)1 / m_sqrt(n2);
#pragma unroll
    for (int j = 0; j < 3; ++j) st[F_EUL + j] = y[Y_Q + j] * rn;
    qd = qq * rn;
#pragma unroll
    for (int j = 0; j < 6; ++j) st[j] = y[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) st[F_OMG + j] = y[Y_W + j];
    // reward and crash: the gym's, on the new position (physics_step_mixed)
    const S dx = st[F_POS + 0] - st[F_TGT + 0];
    const S dy = st[F_POS + 1] - st[F_TGT + 1];
    const S dz = st[F_POS + 2] - st[F_TGT + 2];
    const S dist = m_sqrt((dx * dx + dy * dy) + dz * dz);
    S r = (S)0.01 * -dist;
    if (dist < (S)0.05) r += (S)1;
    const S px = st[F_POS + 0], py = st[F_POS + 1], pz = st[F_POS + 2];
    const S pn2 = (px * px + py * py) + pz * pz;
    crash = (pz < (S)0) || (pn2 > (S)2500);
    return r;
}
template <typename S>
__device__ inline S rk4_h6(const VarArgs<DR_VARIANT_RK4> &va) {
    if constexpr (sizeof(S) == 8) return va.h6d;
    else return va.h6f;
}
// after gym_reset_regs (which zeroes st[3..11]): q = (1, 0, 0, 0)
template <typename S>
__device__ inline void rk4_reset_quat(S st[F_N], S &qd) {
    st[F_EUL] = (S)1;
    qd = (S)0;
}

// Per-wave variant: each wave stages its own 64 rows (3,840 B) and writes
// them out with no workgroup barrier, so a wave delayed by a reset or a late
// load does not hold back the other three waves of its block.
template <int OD, int RPW = 64>
__device__ inline void store_obs_wave(float *sh_block, const float ob[OD],
                                      float *dst_all, int64_t n) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float *sh = sh_block + w * RPW * OD;
    if (lane < RPW) {
#pragma unroll
        for (int k = 0; k < OD; ++k) sh[lane * OD + k] = ob[k];
    }
    // DS ops of one wave execute in order; the barrier only pins the
    // compiler's schedule (no workgroup s_barrier is emitted)
    __builtin_amdgcn_wave_barrier();
    const int64_t wbase = (int64_t)blockIdx.x * (kEnvWpb * RPW) + w * RPW;
    const int64_t nvalid = (n - wbase) < RPW ? (n - wbase) : RPW;
    if (nvalid <= 0) return;
    float *dst = dst_all + wbase * OD;
    if (nvalid == RPW && (((uintptr_t)dst) & 15) == 0) {
        const float4 *s4 = reinterpret_cast<const float4 *>(sh);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
#pragma unroll
        for (int q = lane; q < RPW * OD / 4; q += 64) st_out(&d4[q], s4[q]);
    } else {
        for (int q = lane; q < (int)nvalid * OD; q += 64) dst[q] = sh[q];
    }
}

template <int OD>
__device__ inline void store_obs_block(float *sh, const float ob[OD],
                                       float *dst_all, int64_t base,
                                       int64_t n) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < OD; ++k) sh[tid * OD + k] = ob[k];
    __syncthreads();
    const int64_t nvalid = (n - base) < kBlock ? (n - base) : kBlock;
    float *dst = dst_all + base * OD;
    const int total = (int)nvalid * OD;
    if (nvalid == kBlock && (((uintptr_t)dst) & 15) == 0) {
        const float4 *s4 = reinterpret_cast<const float4 *>(sh);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
#pragma unroll
        for (int q = tid; q < kBlock * OD / 4; q += kBlock) d4[q] = s4[q];
    } else {
        for (int q = tid; q < total; q += kBlock) dst[q] = sh[q];
    }
}

// Element i of a per-env array at a uniform (SGPR) base: the byte offset
// i * sizeof(T) is formed in 32 bits (dr_create caps a handle at 2^28 envs),
// so every SoA access of a wave is one `global_load/store ... v_off, s[base]`
// sharing ONE offset VGPR per element size, with no per-field 64-bit address
// arithmetic ahead of the loads.
template <typename T>
__device__ inline T *at(T *base, int64_t i) {
    return reinterpret_cast<T *>(reinterpret_cast<char *>(base) +
                                 (uint32_t)((uint32_t)i * (uint32_t)sizeof(T)));
}
template <typename T>
__device__ inline const T *at(const T *base, int64_t i) {
    return reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) +
                                       (uint32_t)((uint32_t)i * (uint32_t)sizeof(T)));
}

// ---- a variant's side state ----
// The words an env carries beside st[]: in registers over a step or a rollout
// launch, in memory in the arrays at EnvView::mot (moving: also the centre, in
// the target's arrays).  env_step_kernel and env_rollout_kernel declare one
// Side and call these; what each does for a variant is written here, once.
// SideNone is the variant with no such words (gym, vectorized, tag).  The
// moving variant's centre, motion and target velocity, the smooth variant's
// forces and the wind's mean and gust stay locals of the kernels: wrapped in
// any form (member, reference, always_inline function) moving's instruction
// streams changed, wind's rollout lost a wave of occupancy and smooth's
// changed streams missed the speed check.
template <typename S, int VAR>
struct SideNone {
    // issue the loads, where the kernel's load order has them
    template <bool NTL>
    __device__ void load(const EnvView<S> &, int64_t) {}
    // values formed from the loaded words, once every load is issued
    __device__ void derive() {}
    // "has landed" constraints: of every word (ahead of the rollout's loop),
    // or of those the step has not read before its first store
    __device__ void pin() const {}
    __device__ void pin_late() const {}
    // the words a step changes, written every step or launch
    __device__ void store(const EnvView<S> &, int64_t) const {}
    // the words only a reset (or a reach) changes
    __device__ void store_after_reset(const EnvView<S> &, int64_t) const {}
    // the variant's part of the reset branch, after gym_reset_regs, for env
    // `gid` starting episode `ep_new`
    __device__ void reset(uint32_t, uint32_t, uint64_t, int32_t, const VarArgs<VAR> &, S[F_N]) {}
    // the obs floats past the gym's 15, as make_obs takes them (EXT: has
    // some), and bringing them up to date ahead of an obs
    static constexpr bool EXT = false;
    __device__ const float *ext() const { return nullptr; }
    __device__ void ext_update() {}
};
template <typename S, int VAR>
struct Side : SideNone<S, VAR> {};

// rk4: the quaternion's fourth word (the first three sit in st[F_EUL ..]),
// one array of S, and its f32 for the obs
template <typename S>
struct Side<S, DR_VARIANT_RK4> : SideNone<S, DR_VARIANT_RK4> {
    S qd;
    float qx[1];
    template <bool NTL>
    __device__ void load(const EnvView<S> &v, int64_t i) {
        qd = ld_in<NTL>(at(reinterpret_cast<S *>(v.mot), i));
    }
    __device__ void pin() const { asm volatile("" ::"v"(qd)); }
    __device__ void pin_late() const { pin(); }
    __device__ void store(const EnvView<S> &v, int64_t i) const {
        st_out(at(reinterpret_cast<S *>(v.mot), i), qd);
    }
    __device__ void reset(uint32_t, uint32_t, uint64_t, int32_t,
                          const VarArgs<DR_VARIANT_RK4> &, S st[F_N]) {
        rk4_reset_quat(st, qd);
    }
    static constexpr bool EXT = true;
    __device__ const float *ext() const { return qx; }
    __device__ void ext_update() { qx[0] = (float)qd; }
};

// waypoints: the index within the episode and the reach counter
template <typename S>
struct Side<S, KVAR_WAYPOINT> : SideNone<S, KVAR_WAYPOINT> {
    int32_t j, q;
    template <bool NTL>
    __device__ void load(const EnvView<S> &v, int64_t i) {
        int32_t *const p = reinterpret_cast<int32_t *>(v.mot);
        j = *at(p, i);
        q = *at(p + v.stride, i);
    }
    __device__ void pin() const { asm volatile("" ::"v"(j), "v"(q)); }
    __device__ void pin_late() const { pin(); }
    __device__ void store(const EnvView<S> &v, int64_t i) const {
        int32_t *const p = reinterpret_cast<int32_t *>(v.mot);
        st_out(at(p, i), j);
        st_out(at(p + v.stride, i), q);
    }
    // a new course; q counts on
    __device__ void reset(uint32_t, uint32_t, uint64_t, int32_t, const VarArgs<KVAR_WAYPOINT> &,
                          S[F_N]) {
        j = 0;
    }
};

// airframe: the episode's six words and their two reciprocals; a reset is
// the words' only writer
template <typename S>
struct Side<S, KVAR_AIRFRAME> : SideNone<S, KVAR_AIRFRAME> {
    Airframe af;
    template <bool NTL>
    __device__ void load(const EnvView<S> &v, int64_t i) {
#pragma unroll
        for (int k = 0; k < 6; ++k) af.w[k] = *at(v.mot + k * v.stride, i);
    }
    __device__ void derive() { af.recip(); }
    __device__ void pin() const {
#pragma unroll
        for (int k = 0; k < 6; ++k) asm volatile("" ::"v"(af.w[k]));
    }
    __device__ void store_after_reset(const EnvView<S> &v, int64_t i) const {
#pragma unroll
        for (int k = 0; k < 6; ++k) *at(v.mot + k * v.stride, i) = af.w[k];
    }
    // the new episode's airframe (Philox in host-uniform mode too)
    __device__ void reset(uint32_t k0, uint32_t k1, uint64_t gid, int32_t ep_new,
                          const VarArgs<KVAR_AIRFRAME> &va, S[F_N]) {
        airframe_draw(k0, k1, gid, ep_new, va, af.w);
        af.recip();
    }
};

// HU: reset draws from the host-uniform ring (parity mode).  A template
// parameter, not a runtime branch, so the Philox reset path holds no global
// load: a load there would make the waitcnt pass drain every outstanding
// store of the wave (vmcnt counts stores too) before the reset could finish.
//
// Entry: lanes past the batch end (ragged n, half-populated waves) load the
// last env's row instead of branching around the loads and only their
// stores are masked, so the kernel's first basic block holds every
// kernel-argument load and every state load: one scalar-load round trip
// before the first global load is issued, not two.
template <typename S, int VAR, bool MON, int RPW, bool HU, bool NTL>
__global__ __launch_bounds__(kEnvBlock) void env_step_kernel(EnvView<S> v,
                                                             StepIO io, FieldPtrs<S> fp,
                                                             VarArgs<VAR> va) {
    using T = Traits<VAR>;
    constexpr int OD = T::OD;
    __shared__ float4 sh4[kEnvBlock * OD / 4];
    // Every kernel argument the state loads need is materialised here, in
    // ONE batch of scalar loads: the compiler otherwise issues them in three
    // dependent rounds (n, then the field pointers, then the rest), each a
    // full scalar-memory round trip ahead of the first state load.
    asm volatile("" ::"s"(v.n), "s"(fp.p[0]), "s"(fp.p[1]), "s"(fp.p[2]), "s"(fp.p[3]),
                 "s"(fp.p[4]), "s"(fp.p[5]), "s"(fp.p[6]), "s"(fp.p[7]), "s"(fp.p[8]),
                 "s"(fp.p[9]), "s"(fp.p[10]), "s"(fp.p[11]), "s"(fp.p[12]), "s"(fp.p[13]),
                 "s"(fp.p[14]), "s"(io.actions), "s"(fp.step), "s"(fp.ep_num), "s"(fp.eps));
    __builtin_amdgcn_sched_barrier(0);
    const int64_t n_ = v.n;
    const float4 *const actions = reinterpret_cast<const float4 *>(io.actions);
    int32_t *const p_step = fp.step;
    int32_t *const p_epn = fp.ep_num;
    double *const p_eps = fp.eps;
    const int64_t base = (int64_t)blockIdx.x * (kEnvWpb * RPW);
    const int lane_ = threadIdx.x & 63;
    // env of this lane; lanes >= RPW of a half-populated wave own none
    const int64_t i_own = lane_ < RPW ? base + (threadIdx.x >> 6) * RPW + lane_ : n_;
    const bool live = i_own < n_;
    const int64_t i = live ? i_own : n_ - 1;           // in-bounds row for dead lanes
    DR_STAMP(0);
    float ob[OD];
    S st[F_N];
    int32_t ep_old = 0;
    // Issue order = landing order: euler and omega first so the three
    // sincos range reductions start while pos / vel / target are still in
    // flight (s_waitcnt vmcnt counts oldest-first).
#pragma unroll
    for (int k = F_EUL; k < F_EUL + 3; ++k) st[k] = ld_in<NTL>(at(fp.p[k], i));
    __builtin_amdgcn_sched_barrier(0);     // keep the issue order (euler first)
#pragma unroll
    for (int k = F_OMG; k < F_OMG + 3; ++k) st[k] = ld_in<NTL>(at(fp.p[k], i));
    const float4 act = *at(actions, i);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < F_EUL; ++k) st[k] = ld_in<NTL>(at(fp.p[k], i));
    S cen[3];
    float mp[9], tvel[3];           // moving: centre, motion, target velocity
    float wm[3], wg[3];             // wind: the episode's mean wind, the gust
    float fm[4];                    // smooth: the motor forces
    Side<S, VAR> sd;                // the other variants' side words
    float dev_sq = 0.f;             // smooth: |command - force|^2
    // tag: the partner's position / velocity, the obs past the first 12, the
    // role (env ids 2j pursue; i and env_id_offset + i have one parity)
    S pp[3], pv[3];
    float tx[7];
    const bool pursuer = (i & 1) == 0;
    const float sigma = pursuer ? 1.0f : -1.0f;
    sd.template load<NTL>(v, i);
    if constexpr (T::SMOOTH) {
#pragma unroll
        for (int k = 0; k < 4; ++k) fm[k] = *at(v.mot + k * v.stride, i);
    }
    if constexpr (T::WIND) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            wm[k] = *at(v.mot + k * v.stride, i);
            wg[k] = *at(v.mot + (3 + k) * v.stride, i);
        }
    }
    if constexpr (T::TAG) {
        // nothing in the step reads the stored target: a reset writes it
#pragma unroll
        for (int k = F_TGT; k < F_N; ++k) st[k] = (S)0;
    } else if constexpr (T::GYMSTATE) {
#pragma unroll
        for (int k = F_TGT; k < F_N; ++k) st[k] = ld_in<NTL>(at(fp.p[k], i));
    } else if constexpr (T::MOVING) {
#pragma unroll
        for (int k = 0; k < 3; ++k) cen[k] = *at(fp.p[F_TGT + k], i);
#pragma unroll
        for (int k = 0; k < 9; ++k) mp[k] = *at(v.mot + k * v.stride, i);
    } else {
        st[F_TGT + 0] = (S)0;
        st[F_TGT + 1] = (S)0;
        st[F_TGT + 2] = (S)10.0;
    }
    int32_t step = ld_in<NTL>(at(p_step, i));
    // needed only if this env resets; loaded up front so a reset does not
    // stall the wave on a dependent global load (+12 B per step, counted in
    // the measured traffic, not in the 305 B algorithmic)
    double eps_old = 0.0;
    if constexpr (T::GYMLIKE) {
        ep_old = *at(p_epn, i);
        // eps loaded with the state: the Philox reset path holds no global
        // load (6-8 % faster at 65,536-131,072 envs than loading it in the reset)
        eps_old = *at(p_eps, i);
    }
    // VecMonitor counters: also loaded up front (a load after the physics
    // would put one more full memory latency on every wave)
    float ret0 = 0.f;
    int32_t len0 = 0;
    if constexpr (MON) {
        ret0 = *at(v.ep_ret, i);
        len0 = *at(v.ep_len, i);
    }
    // Every load is issued before any arithmetic: without this the
    // scheduler interleaves the first sincos with the loads and its
    // s_waitcnt holds back the issue of the remaining ones by a full memory
    // latency.
    __builtin_amdgcn_sched_barrier(0);
    sd.derive();
    if constexpr (T::MOVING) {
        // the reward and obs of this step see the target at the NEW step
        moving_target(cen, mp, step + 1, (float)v.dt, &st[F_TGT], tvel);
    }

    // the gust and the drag impulse sit in front of the gym step, on the
    // step counter and episode the step starts from
    if constexpr (T::WIND)
        wind_pre<S>(st, wm, wg, va, v.seed_lo, v.seed_hi, (uint64_t)(v.env_id_offset + i), ep_old,
                    step, v.dt);
    bool crash;
    bool reached = false;
    S r;
    if constexpr (T::SMOOTH) {
        // the physics sees the lagged forces, not the command
        r = physics_step<S, VAR>(st, smooth_filter(act, fm, va.alpha, dev_sq), v.dt, crash);
    } else if constexpr (T::RK4) {
        r = rk4_step<S>(st, sd.qd, motor_mix(act), v.dt, rk4_h6<S>(va), crash);
    } else if constexpr (T::WAYPT) {
        r = physics_step<S, VAR>(st, act, v.dt, crash, &va, &reached);
    } else if constexpr (T::AIRF) {
        // the motor mixes of the gained command, the physics on 1/m and 1/s
        r = physics_step<S, VAR>(st, airframe_gain(sd.af, act), v.dt, crash, nullptr, nullptr,
                                 &sd.af);
    } else {
        r = physics_step<S, VAR>(st, act, v.dt, crash);
    }
    DR_STAMP(2);
    step += 1;                                             // (155)
    bool done, any_crash = crash;   // any_crash: own or (tag) the partner's
    if constexpr (T::TAG) {
        // Wave-uniform code (dead lanes ran the physics on row n - 1, and
        // their partners are dead too): exchange the new position and
        // velocity and the own crash / done flags, then the pair's reward
        // and its common end.
        const int own = (int)crash | ((int)(crash || (step >= v.max_steps)) << 1);
        tag_partner(st, pp, pv);
        const int oth = partner_of(own);
        r = tag_reward(st, pp, va.radius, pursuer);
        any_crash = crash || (oth & 1);
        done = live && (((own | oth) & 2) != 0);
    } else {
        done = live && (crash || (step >= v.max_steps));   // (156-157)
    }
    float rf = (float)r;                                   // SB3 f32 buffer
    if constexpr (T::SMOOTH) {
        // uniform branch: at lam == 0 the reward is the gym's even where
        // dev_sq overflowed
        if (va.lam != 0.f) rf = rf - va.lam * dev_sq;
    }
    if constexpr (T::TAG) {
        // uniform branch, one f32 subtract for the lanes that crashed
        if (va.crash != 0.f) rf = crash ? rf - va.crash : rf;
    }
    // Every value loaded up front has landed before the first store is
    // issued (they were issued first and the physics took longer than
    // their latency, so this waits for nothing).  Without it the compiler
    // places the waits for the late-used ones (ep_num / eps in the reset
    // branch, the VecMonitor counters, the step counter) at their uses,
    // after the rew / done (and terminal obs) stores: vmcnt(0) there drains
    // those stores as well -- vmcnt counts both, in issue order -- once
    // in the reset branch and again where it rejoins, for every wave.
    asm volatile("" ::"v"(step), "v"(ep_old), "v"(eps_old), "v"(ret0), "v"(len0));
#pragma unroll
    for (int k = 0; k < (T::TAG ? 12 : F_N); ++k) asm volatile("" ::"v"(st[k]));
    sd.pin_late();
    if (live) {
        st_out(at(io.rew, i), rf);
        st_out(at(io.done, i), (uint8_t)done);
    }
    if constexpr (T::WAYPT) {
        // the course moves on, ahead of the terminal obs and of a reset
        // (which overwrites the target it stores)
        if (reached && live) {
            sd.j += 1;
            sd.q += 1;
            waypoint_draw<S>(st, v.seed_lo, v.seed_hi, (uint64_t)(v.env_id_offset + i), ep_old,
                             eps_old, sd.j);
#pragma unroll
            for (int k = F_TGT; k < F_N; ++k) *at(fp.p[k], i) = st[k];
        }
    }

    float ret = 0.f;
    int32_t len = 0;
    if constexpr (MON) {
        ret = ret0 + rf;                                   // VecMonitor
        len = len0 + 1;
    }
    if constexpr (T::GYMLIKE) {
        if (done && io.auto_reset) {
            // DummyVecEnv: keep the terminal obs, reset in the same step.
            if (io.term_obs) {
                // tag: the partner's terminal state, exchanged before the branch
                if constexpr (T::TAG) tag_ext(st, pp, pv, sigma, tx);
                sd.ext_update();
                make_obs<S, VAR>(st, ob, T::TAG ? tx : (T::MOVING ? tvel : (T::SMOOTH ? fm : sd.ext())));
#pragma unroll
                for (int k = 0; k < OD; ++k) io.term_obs[i * OD + k] = ob[k];
            }
            step = 0;
            if constexpr (T::GYMSTATE) {
                gym_reset_regs(v, i, HU ? 1 : 0, st, ep_old, eps_old);
                sd.reset(v.seed_lo, v.seed_hi, (uint64_t)(v.env_id_offset + i), ep_old + 1, va, st);
                sd.store_after_reset(v, i);
                if constexpr (T::WIND) {
                    // the new episode's mean wind (Philox in host-uniform
                    // mode too), still air around it
                    wind_mean(v.seed_lo, v.seed_hi, (uint64_t)(v.env_id_offset + i), ep_old + 1,
                              va.W, wm);
#pragma unroll
                    for (int k = 0; k < 3; ++k) wg[k] = 0.f;
                }
#pragma unroll
                for (int k = F_TGT; k < F_N; ++k) *at(fp.p[k], i) = st[k];
                if constexpr (T::SMOOTH) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) fm[k] = kHover32;
                }
            } else {
                moving_reset_regs(v, i, HU ? 1 : 0, st, cen, mp, ep_old, eps_old);
#pragma unroll
                for (int k = 0; k < 3; ++k) *at(fp.p[F_TGT + k], i) = cen[k];
#pragma unroll
                for (int k = 0; k < 9; ++k) *at(v.mot + k * v.stride, i) = mp[k];
                moving_target(cen, mp, 0, (float)v.dt, &st[F_TGT], tvel);
            }
        }
    }
    if constexpr (T::TAG) {
        // The reset branch has rejoined: the partner's state once more, now
        // post-reset (both members of a pair reset in the same step).  Skipped,
        // wave-uniformly, when no lane reset: the values are those of the
        // first exchange.
        if (__any(done && io.auto_reset)) tag_partner(st, pp, pv);
        tag_ext(st, pp, pv, sigma, tx);
    }
    // ONE observation pass over the post-reset state (the terminal obs is
    // formed inside the reset branch only when the caller keeps it)
    sd.ext_update();
    make_obs<S, VAR>(st, ob, T::TAG ? tx : (T::MOVING ? tvel : (T::SMOOTH ? fm : sd.ext())));
    if constexpr (MON) {
        if (io.trunc_out && live) *at(io.trunc_out, i) = (uint8_t)(done && !any_crash);
        if (done) {               // VecMonitor: report, then restart counters
            *at(io.ep_ret_out, i) = ret;
            *at(io.ep_len_out, i) = len;
            ret = 0.f;
            len = 0;
        }
        if (live) {
            *at(v.ep_ret, i) = ret;
            *at(v.ep_len, i) = len;
        }
    }
    DR_STAMP(3);
    if (live) {
#pragma unroll
        for (int k = 0; k < 12; ++k) st_out(at(fp.p[k], i), st[k]);
        st_out(at(p_step, i), step);
        sd.store(v, i);
        if constexpr (T::SMOOTH) {
#pragma unroll
            for (int k = 0; k < 4; ++k) st_out(at(v.mot + k * v.stride, i), fm[k]);
        }
        if constexpr (T::WIND) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                st_out(at(v.mot + k * v.stride, i), wm[k]);
                st_out(at(v.mot + (3 + k) * v.stride, i), wg[k]);
            }
        }
    }
    DR_STAMP(4);
    if (!live) {
#pragma unroll
        for (int k = 0; k < OD; ++k) ob[k] = 0.f;
    }
    store_obs_wave<OD, RPW>(reinterpret_cast<float *>(sh4), ob, io.obs, v.n);
    DR_STAMP(5);
}

// ----------------------------------------------------------------------------
// K-step rollout: K successive steps of the same batch in ONE launch, the
// state held in registers between steps.  Equivalent, output for output and
// bit for bit, to K env_step_kernel launches (dr_step with no terminal obs,
// no VecMonitor) on actions[t] -- or, GEN, on the random policy's actions
// generated in-kernel with random_actions_kernel's exact Philox draw for
// step step0 + t.  This is the random-policy rollout loop (a = sample();
// obs, r, done = env.step(a), K times; drone.py:81-159 per step, the
// DummyVecEnv auto-reset in between) with the per-step state round trip
// through HBM and the per-launch gap removed: per env-step it moves the
// outputs (obs 4*OD + rew 4 + done 1 B) and the action (16 B, none when
// GEN), plus the state once per launch.
//
// Every step's outputs are stored as they are formed (rew / done per lane,
// obs through the per-wave LDS staging), so the stores of step t drain
// while step t+1 computes; actions are loaded two steps ahead.  The fields
// a reset changes outside the 12 dynamic ones (target,
// motion; ep_num / eps are written by the reset itself) are written back
// at the end only for lanes that reset during the launch.
// ----------------------------------------------------------------------------
struct RolloutIO {
    const float *actions;   // (K, n, 4); unused when GEN
    float *act_out;         // GEN: optional (K, n, 4) copy of the drawn actions
    float *obs;             // (K, n, OD)
    float *rew;             // (K, n)
    uint8_t *done;          // (K, n)
    int32_t k;
    uint32_t a_k0, a_k1;    // action Philox key
    uint64_t a_step0;
    float a_lo, a_span;
    int auto_reset;
};

// The random policy's action of env `gid` at policy step `s`: one Philox word
// per env and step under the key (k0, k1), scaled to [lo, lo + span).  The
// rollout kernels re-declare the key opaque at every draw themselves (see
// env_rollout_kernel): with that pin inside this function their device code
// changed.
__device__ inline float4 action_of(uint64_t s, uint64_t gid, uint32_t k0, uint32_t k1,
                                   float lo, float span) {
    const u32x4 r = philox4x32_10(
        u32x4{(uint32_t)s, (uint32_t)(s >> 32), (uint32_t)gid, TAG_ACTION ^ (uint32_t)(gid >> 32)},
        k0, k1);
    return make_float4(lo + span * u01_f32(r.x), lo + span * u01_f32(r.y),
                       lo + span * u01_f32(r.z), lo + span * u01_f32(r.w));
}

template <typename S, int VAR, int RPW, bool GEN>
__global__ __launch_bounds__(kEnvBlock) void env_rollout_kernel(EnvView<S> v, RolloutIO io,
                                                                FieldPtrs<S> fp,
                                                                VarArgs<VAR> va) {
    using T = Traits<VAR>;
    constexpr int OD = T::OD;
    __shared__ float4 sh4[kEnvBlock * OD / 4];
    const int64_t n_ = v.n;
    const int64_t base = (int64_t)blockIdx.x * (kEnvWpb * RPW);
    const int lane_ = threadIdx.x & 63;
    const int64_t i_own = lane_ < RPW ? base + (threadIdx.x >> 6) * RPW + lane_ : n_;
    const bool live = i_own < n_;
    const int64_t i = live ? i_own : n_ - 1;
    const uint64_t gid = (uint64_t)(v.env_id_offset + i);
    S st[F_N];
#pragma unroll
    for (int k = F_EUL; k < F_N - 3; ++k) st[k] = *at(fp.p[k], i);
#pragma unroll
    for (int k = 0; k < F_EUL; ++k) st[k] = *at(fp.p[k], i);
    S cen[3];
    float mp[9], tvel[3];
    // the variant's side words, carried in registers over the launch like
    // the rest of the state (airframe: with the two reciprocals)
    Side<S, VAR> sd;
    float wm[3], wg[3];    // wind: the mean wind and the gust, likewise
    float fm[4];           // smooth: the motor forces, likewise
    float dev_sq = 0.f;    // smooth: this step's |command - force|^2
    // tag: the obs past the first 12 and the role (env_step_kernel)
    float tx[7];
    const bool pursuer = (i & 1) == 0;
    const float sigma = pursuer ? 1.0f : -1.0f;
    // the obs past the gym's 15 (tvel: the moving variant's; unread elsewhere)
    const float *const ext =
        T::TAG ? tx : (T::SMOOTH ? fm : (Side<S, VAR>::EXT ? sd.ext() : tvel));
    sd.template load<false>(v, i);
    sd.derive();
    if constexpr (T::SMOOTH) {
#pragma unroll
        for (int k = 0; k < 4; ++k) fm[k] = *at(v.mot + k * v.stride, i);
    }
    if constexpr (T::WIND) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            wm[k] = *at(v.mot + k * v.stride, i);
            wg[k] = *at(v.mot + (3 + k) * v.stride, i);
        }
    }
    if constexpr (T::GYMSTATE) {
#pragma unroll
        for (int k = F_TGT; k < F_N; ++k) st[k] = *at(fp.p[k], i);
    } else if constexpr (T::MOVING) {
#pragma unroll
        for (int k = 0; k < 3; ++k) cen[k] = *at(fp.p[F_TGT + k], i);
#pragma unroll
        for (int k = 0; k < 9; ++k) mp[k] = *at(v.mot + k * v.stride, i);
    } else {
        st[F_TGT + 0] = (S)0;
        st[F_TGT + 1] = (S)0;
        st[F_TGT + 2] = (S)10.0;
    }
    int32_t step = *at(fp.step, i);
    int32_t ep_num = 0;
    double eps = 0.0;
    if constexpr (T::GYMLIKE) {
        ep_num = *at(fp.ep_num, i);
        eps = *at(fp.eps, i);
    }
    bool reset_any = false;
    float ob[OD];

    // The Philox keys (reset draws; GEN: actions) are re-declared opaque
    // once per step, so the compiler cannot hoist the 10-round key
    // schedules out of the loop: hoisted, their 40 words spilled to VGPR
    // lanes, and every round paid a v_readlane plus a hazard s_nop.
    EnvView<S> vk = v;
    // The Philox blocks of a lane's NEXT reset (episode ep_num + 1; gym:
    // block 0 = pos x, y and target x, y; moving: all four) are drawn ahead, for every lane
    // whose draw is used up, at the first step of each group of
    // kResetAhead steps -- a wave-wide pass once per group instead of the
    // reset branch's Philox, which a wave runs at almost every step (≈86 % of
    // waves hold a resetting env at each step under the random policy).  A
    // lane resetting twice within one group draws in the branch as before;
    // the draws are the same Philox words either way.
    constexpr int NB = T::NB;
    u32x4 nd[NB] = {};
    bool nd_ok = false;
    // (Traits::SIDE_AHEAD, the airframe: the next episode's six words and two
    // reciprocals ride with them, so the branch holds neither their two Philox
    // blocks nor the two divides; the values are the same either way)
    Side<S, VAR> sdn;
    // the step limit in a VGPR: under the kernel's SGPR pressure the
    // compiler otherwise re-reads it from the kernel arguments at every
    // step (a scalar load and its wait on the critical path)
    int32_t max_steps;
    asm volatile("v_mov_b32 %0, %1" : "=v"(max_steps) : "s"(v.max_steps));
    // one step from the action's motor mixes: the body of env_step_kernel
    // on registers
    // the motor mixes the physics sees for command `act`: the command's own,
    // or (smooth) those of the lagged forces, which the lag updates here
    auto mix_of = [&](const float4 act) -> MotorMix {
        if constexpr (T::SMOOTH) return motor_mix(smooth_filter(act, fm, va.alpha, dev_sq));
        else if constexpr (T::AIRF) return motor_mix(airframe_gain(sd.af, act));
        else return motor_mix(act);
    };
    auto step_one = [&](const MotorMix mx, const int t) {
        asm volatile("" : "+s"(vk.seed_lo), "+s"(vk.seed_hi));
        if constexpr (T::GYMLIKE) {
            if (t % kResetAhead == 0 && !nd_ok) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    nd[b] = philox4x32_10(u32x4{(uint32_t)(ep_num + 1), (uint32_t)gid,
                                                (uint32_t)(gid >> 32), TAG_RESET | (uint32_t)b},
                                          vk.seed_lo, vk.seed_hi);
                if constexpr (T::SIDE_AHEAD)
                    sdn.reset(vk.seed_lo, vk.seed_hi, gid, ep_num + 1, va, st);
                nd_ok = true;
            }
        }
        if constexpr (T::MOVING)
            moving_target(cen, mp, step + 1, (float)v.dt, &st[F_TGT], tvel);
        if constexpr (T::WIND)
            wind_pre<S>(st, wm, wg, va, vk.seed_lo, vk.seed_hi, gid, ep_num, step, v.dt);
        bool crash;
        bool reached = false;
        S r;
        if constexpr (T::RK4) r = rk4_step<S>(st, sd.qd, mx, v.dt, rk4_h6<S>(va), crash);
        else if constexpr (T::WAYPT)
            r = physics_step_mixed<S, VAR>(st, mx, v.dt, crash, &va, &reached);
        else if constexpr (T::AIRF)
            r = physics_step_mixed<S, VAR>(st, mx, v.dt, crash, nullptr, nullptr, &sd.af);
        else r = physics_step_mixed<S, VAR>(st, mx, v.dt, crash);
        step += 1;
        bool done;
        S pp[3], pv[3];
        if constexpr (T::TAG) {
            // wave-uniform: the exchanges of env_step_kernel, all in registers
            // (no global store is added to the step)
            const int own = (int)crash | ((int)(crash || (step >= max_steps)) << 1);
            tag_partner(st, pp, pv);
            const int oth = partner_of(own);
            r = tag_reward(st, pp, va.radius, pursuer);
            done = live && (((own | oth) & 2) != 0);
        } else {
            done = live && (crash || (step >= max_steps));
        }
        const int64_t row = (int64_t)t * n_;
        if (live) {
            if constexpr (T::TAG) {
                float rf = (float)r;
                if (va.crash != 0.f) rf = crash ? rf - va.crash : rf;
                st_out(at(io.rew + row, i), rf);
            } else if constexpr (T::SMOOTH) {
                float rf = (float)r;
                // uniform branch, as in env_step_kernel
                if (va.lam != 0.f) rf = rf - va.lam * dev_sq;
                st_out(at(io.rew + row, i), rf);
            } else {
                st_out(at(io.rew + row, i), (float)r);
            }
            st_out(at(io.done + row, i), (uint8_t)done);
        }
        if constexpr (T::WAYPT) {
            // the course moves on (env_step_kernel), all in registers; the
            // target is written back at the end, as after a reset
            if (reached && live) {
                sd.j += 1;
                sd.q += 1;
                waypoint_draw<S>(st, vk.seed_lo, vk.seed_hi, gid, ep_num, eps, sd.j);
                reset_any = true;
            }
        }
        if constexpr (T::GYMLIKE) {
            if (done && io.auto_reset) {
                step = 0;
                reset_any = true;
                if constexpr (T::GYMSTATE) {
                    if constexpr (T::SIDE_AHEAD) {
                        if (nd_ok) sd = sdn;
                        else sd.reset(vk.seed_lo, vk.seed_hi, gid, ep_num + 1, va, st);
                    }
                    gym_reset_regs(vk, i, 0, st, ep_num, eps, nd_ok ? &nd[0] : nullptr);
                    nd_ok = false;
                    if constexpr (T::SIDE && !T::SIDE_AHEAD)
                        sd.reset(vk.seed_lo, vk.seed_hi, gid, ep_num + 1, va, st);
                    if constexpr (T::SMOOTH) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) fm[k] = kHover32;
                    }
                    if constexpr (T::WIND) {
                        wind_mean(vk.seed_lo, vk.seed_hi, gid, ep_num + 1, va.W, wm);
#pragma unroll
                        for (int k = 0; k < 3; ++k) wg[k] = 0.f;
                    }
                } else {
                    moving_reset_regs(vk, i, 0, st, cen, mp, ep_num, eps, nd_ok ? nd : nullptr);
                    nd_ok = false;
                    moving_target(cen, mp, 0, (float)v.dt, &st[F_TGT], tvel);
                }
                // the curriculum counters gym/moving_reset_regs just wrote
                // (drone.py:61, 68-70), carried on in registers
                ep_num += 1;
                if (ep_num % 2000 == 0) eps += 0.1;
            }
        }
        if constexpr (T::TAG) {
            // rejoined: the partner's post-reset state (env_step_kernel)
            if (__any(done && io.auto_reset)) tag_partner(st, pp, pv);
            tag_ext(st, pp, pv, sigma, tx);
        }
        if constexpr (Side<S, VAR>::EXT) sd.ext_update();
        make_obs<S, VAR>(st, ob, ext);
        if (!live) {
#pragma unroll
            for (int k = 0; k < OD; ++k) ob[k] = 0.f;
        }
        // (plain stores for these outputs measured the same: 60.2 / 62.2 us
        // per 32-step launch at 65,536 envs)
        store_obs_wave<OD, RPW>(reinterpret_cast<float *>(sh4), ob, io.obs + row * OD, n_);
    };

    if constexpr (GEN) {
        for (int t = 0; t < io.k; ++t) {
            const uint64_t s = io.a_step0 + (uint64_t)t;
            uint32_t ak0 = io.a_k0, ak1 = io.a_k1;
            asm volatile("" : "+s"(ak0), "+s"(ak1));
            const float4 act = action_of(s, gid, ak0, ak1, io.a_lo, io.a_span);
            if (io.act_out && live)
                st_out(at(reinterpret_cast<float4 *>(io.act_out) + (int64_t)t * n_, i), act);
            step_one(mix_of(act), t);
        }
    } else {
        // Each action is loaded ahead into the registers the action two
        // steps earlier just vacated (right after its motor mixes, its only
        // use), by an asm load the compiler does not track: its own waitcnt
        // pass, at a loop back edge, waits vmcnt(0) for any load in flight
        // -- draining every store of the step as well (vmcnt counts both,
        // in issue order).  The hand-placed wait below counts only stores
        // that a wave with a live lane always issues (a wave with none
        // stores nothing and its lanes' results are discarded).  The first
        // two actions are ordinary loads.
        typedef float f4v __attribute__((ext_vector_type(4)));
        const float4 *const acts = reinterpret_cast<const float4 *>(io.actions);
        const float4 a_first = *at(acts, i);
        const float4 b_first = io.k > 1 ? *at(acts + n_, i) : a_first;
        f4v a = {a_first.x, a_first.y, a_first.z, a_first.w};
        f4v b = {b_first.x, b_first.y, b_first.z, b_first.w};
        // every preheader load landed before the loop: otherwise the
        // compiler places the waits for them at their first uses inside
        // the loop (ep_num / eps in the reset branch, a state component in
        // the physics), where they run every step as vmcnt(0)
        asm volatile("" ::"v"(ep_num), "v"(eps), "v"(a), "v"(b), "v"(step));
#pragma unroll
        for (int k = 0; k < F_N; ++k) asm volatile("" ::"v"(st[k]));
        sd.pin();
        if constexpr (T::SMOOTH) {
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("" ::"v"(fm[k]));
        }
        if constexpr (T::WIND) {
#pragma unroll
            for (int k = 0; k < 3; ++k) asm volatile("" ::"v"(wm[k]), "v"(wg[k]));
        }
        if constexpr (T::MOVING) {
#pragma unroll
            for (int k = 0; k < 3; ++k) asm volatile("" ::"v"(cen[k]));
#pragma unroll
            for (int k = 0; k < 9; ++k) asm volatile("" ::"v"(mp[k]));
        }
        // Two steps ahead, in two registers that alternate (the loop is
        // unrolled by two so each keeps its role): step t's action was
        // loaded at the top of step t-2; younger than that load are step
        // t-2's rew / done stores, step t-1's action load (when issued) and
        // step t-1's rew / done stores, so vmcnt(4) waits for it and no
        // further.  One step ahead left part of the HBM latency exposed
        // (62.9 us per 32-step launch with 335 MB of distinct actions
        // against 50.5 with one cache-resident action set).
        auto act_step = [&](f4v &r, const int t) {
            if (t >= 2) {
                // younger than step t's action load (issued at the top of step
                // t - 2): each of steps t - 2 and t - 1 issues its reward,
                // done and NQ obs-row stores, step t - 1 the next load
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            }
            const MotorMix mx = mix_of(make_float4(r.x, r.y, r.z, r.w));
            asm volatile("" ::"v"(mx.thr), "v"(mx.phi), "v"(mx.theta), "v"(mx.psi));
            __builtin_amdgcn_sched_barrier(0);
            if (t + 2 < io.k) {
                const float4 *pa = at(acts + (int64_t)(t + 2) * n_, i);
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(pa) : "memory");
            }
            __builtin_amdgcn_sched_barrier(0);
            step_one(mx, t);
        };
        for (int t = 0; t < io.k; t += 2) {
            act_step(a, t);
            if (t + 1 < io.k) act_step(b, t + 1);
        }
        // a wave with no live lane never waited for its loads: none may
        // still be writing registers the code below reuses
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < 12; ++k) st_out(at(fp.p[k], i), st[k]);
        st_out(at(fp.step, i), step);
        sd.store(v, i);
        if constexpr (T::SMOOTH) {
#pragma unroll
            for (int k = 0; k < 4; ++k) st_out(at(v.mot + k * v.stride, i), fm[k]);
        }
        if constexpr (T::WIND) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                st_out(at(v.mot + k * v.stride, i), wm[k]);
                st_out(at(v.mot + (3 + k) * v.stride, i), wg[k]);
            }
        }
        // (waypoints: or reached a waypoint, which moves the target too)
        if (reset_any) {
            if constexpr (T::GYMSTATE) {
#pragma unroll
                for (int k = F_TGT; k < F_N; ++k) *at(fp.p[k], i) = st[k];
                sd.store_after_reset(v, i);
            } else if constexpr (T::MOVING) {
#pragma unroll
                for (int k = 0; k < 3; ++k) *at(fp.p[F_TGT + k], i) = cen[k];
#pragma unroll
                for (int k = 0; k < 9; ++k) *at(v.mot + k * v.stride, i) = mp[k];
            }
        }
    }
}

// ----------------------------------------------------------------------------
// Warp-specialised K-step rollout (dr_rollout's default launch form).
// 512-thread blocks of 256 envs: waves 0-3, the PHYSICS waves (one per SIMD),
// run the steps on registers exactly as env_rollout_kernel does, with no
// global load inside the step loop (its only global stores are a reset's
// ep_num / eps); waves 4-7, the MEMORY waves
// (wave p + 4 shares SIMD p with physics wave p), move the bytes: each loads
// its partner's actions by LDS-DMA kWsAhead + 1 steps ahead into a ring of
// LDS slots (GEN: draws the random policy's actions into them), and streams
// its partner's finished outputs -- obs rows, reward, done, staged in LDS by
// the physics wave -- to HBM.  One s_barrier per step hands the slots over.  At one physics wave per SIMD, env_rollout_kernel's
// wave issues its own stores and action loads between steps (the write
// stream alone is ~0.9 us per step at 65,536 envs); here
// that issue and its back-pressure sit on the memory waves, beside the
// physics.
//
// Outputs are bitwise those of env_rollout_kernel (the same physics, reset
// and Philox code on the same registers; only where the bytes travel
// differs); tests/test_rollout_gpu.py checks both forms against K dr_step.
//
// Step t / phase t (B_t = the barrier that ends physics step t):
//   physics: action t from slot t % NA (landed before B_(t-1)), the step,
//            outputs into slot t & 1, lgkmcnt(0), B_t
//   memory:  after B_(t-1): LDS-DMA action t + D + 1 into slot (t + D + 1) % NA
//            (its previous action, t - 1, was read before B_(t-1)); load
//            slot (t - 1) & 1 and store it to HBM (physics writes that slot
//            again only after B_t); wait for action t + 1 (vmcnt, counted by
//            hand: vmcnt counts loads and stores in issue order), B_t.
//   After the last barrier the memory waves store step K - 1's outputs.
// ----------------------------------------------------------------------------
constexpr int kWsEnvs = 256;                 // envs per block: 4 physics waves
constexpr int kWsThreads = 2 * kWsEnvs;
// D: how many steps ahead of the physics the memory waves issue an action
// load (the physics wave reads action t at the top of step t; the
// hand-counted waits below are generic in D; vmcnt holds at most 63, so
// S_OPS + D * (S_OPS + 1) must stay below it).  Ring slots: D + 2.
constexpr int kWsAhead = 2;                  // D
constexpr int kWsNA = kWsAhead + 2;          // action ring slots


// global_load_lds_dwordx4: lane l's 16 bytes land at LDS byte lds_base + 16 l
// (the wave's 64 actions as one 1-KB slot).  It clobbers m0, which the
// compiler reserves (and sets before each of its own uses).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ inline void ws_glds16(const void *gptr, uint32_t lds_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
                 ::"v"(gptr), "s"(lds_base)
                 : "memory", "m0");
}
#pragma clang diagnostic pop


template <int OD>
struct WsLds {
    float obs[2][kWsEnvs * OD];              // per slot: 4 waves x 64 rows x OD
    float rew[2][kWsEnvs];
    uint8_t done[2][kWsEnvs];
    float4 act[kWsNA][kWsEnvs];
};

template <typename S, int VAR, bool GEN>
__global__ __launch_bounds__(kWsThreads) void env_rollout_ws_kernel(EnvView<S> v, RolloutIO io,
                                                                    FieldPtrs<S> fp) {
    using T = Traits<VAR>;
    constexpr int OD = T::OD;
    constexpr int NQ = (64 * OD / 4 + 63) / 64;  // float4 rows-stores per lane and step
    // the hand-counted wait assumes NQ obs + 1 reward + 1 done store per phase
    constexpr int S_OPS = NQ + 2;
    static_assert(S_OPS + kWsAhead * (S_OPS + 1) <= 63,
                  "the action-load wait count must fit vmcnt");
    __shared__ __attribute__((aligned(16))) WsLds<OD> sh;
    const int64_t n_ = v.n;
    const int K = io.k;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = wid & 3;                        // physics wave / partner index
    const int64_t wbase = (int64_t)blockIdx.x * kWsEnvs + p * 64;
    const int64_t i_own = wbase + lane;
    const bool live = i_own < n_;
    const int64_t i = live ? i_own : n_ - 1;

    if (wid >= 4) {
        // ---------------- memory wave ----------------
        const int64_t nvalid = (n_ - wbase) < 64 ? (n_ - wbase) : 64;
        // full: 64 live rows and 16-byte aligned obs rows at every step; else
        // (the ragged last wave) scalar stores and vmcnt(0) waits
        const bool full = nvalid == 64 && (((uintptr_t)io.obs) & 15) == 0 &&
                          ((n_ * OD) & 3) == 0;
        const float4 *acts = reinterpret_cast<const float4 *>(io.actions);
        // GEN: the memory wave draws the random policy's action itself
        // (random_actions_kernel's Philox word for step a_step0 + t) into the
        // slot, off the physics wave's instruction stream
        const uint64_t gid = (uint64_t)(v.env_id_offset + i);
        auto load_act = [&](int t) {
            if constexpr (GEN) {
                const uint64_t s = io.a_step0 + (uint64_t)t;
                uint32_t ak0 = io.a_k0, ak1 = io.a_k1;
                asm volatile("" : "+s"(ak0), "+s"(ak1));
                const float4 act = action_of(s, gid, ak0, ak1, io.a_lo, io.a_span);
                sh.act[t % kWsNA][p * 64 + lane] = act;
                if (io.act_out && live)
                    st_out(at(reinterpret_cast<float4 *>(io.act_out) + (int64_t)t * n_, i), act);
            } else if (nvalid > 0) {
                ws_glds16(at(acts + (int64_t)t * n_, i),
                          (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)
                              &sh.act[t % kWsNA][p * 64]);
            }
        };
        auto store_out = [&](int t) {
            if (nvalid <= 0) return;
            const int so = t & 1;
            const int64_t row = (int64_t)t * n_;
            const float *src = &sh.obs[so][p * 64 * OD];
            float *dst = io.obs + (row + wbase) * OD;
            const float r = sh.rew[so][p * 64 + lane];
            const uint8_t d = sh.done[so][p * 64 + lane];
            if (full) {
                float4 q[NQ];
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    if (j * 64 + lane < 64 * OD / 4)
                        q[j] = reinterpret_cast<const float4 *>(src)[j * 64 + lane];
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    if (j * 64 + lane < 64 * OD / 4)
                        st_out(reinterpret_cast<float4 *>(dst) + j * 64 + lane, q[j]);
            } else {
                for (int q = lane; q < (int)nvalid * OD; q += 64) st_out(dst + q, src[q]);
            }
            if (live) {
                st_out(at(io.rew + row, i_own), r);
                st_out(at(io.done + row, i_own), d);
            }
        };
        for (int t = 0; t <= kWsAhead && t < K; ++t) load_act(t);
        if (!GEN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // actions 0 .. D
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_(-1)
        for (int t = 0; t < K; ++t) {
            if (t + kWsAhead + 1 < K) load_act(t + kWsAhead + 1);
            if (t >= 1) store_out(t - 1);
            // action a = t + 1 must have landed before B_t (actions 0 .. D
            // did before B_(-1)).  It was issued first in phase q = a - D - 1
            // = t - D; younger in the steady state: q's S_OPS stores and D
            // phases of one load and S_OPS stores; elsewhere at least this
            // phase's S_OPS stores (t >= 1 here).  A ragged wave waits for
            // every op.
            constexpr int AH = kWsAhead;
            if (!GEN && t + 1 < K && t + 1 > kWsAhead) {
                __builtin_amdgcn_sched_barrier(0);
                if (!full)
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (t >= AH + 1 && t + kWsAhead + 1 < K)
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S_OPS + AH * (S_OPS + 1))
                                 : "memory");
                else
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S_OPS) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_t
        }
        if (K > 0) store_out(K - 1);
        return;
    }

    // ---------------- physics wave ----------------
    const uint64_t gid = (uint64_t)(v.env_id_offset + i);
    S st[F_N];
#pragma unroll
    for (int k = F_EUL; k < F_N - 3; ++k) st[k] = *at(fp.p[k], i);
#pragma unroll
    for (int k = 0; k < F_EUL; ++k) st[k] = *at(fp.p[k], i);
    S cen[3];
    float mp[9], tvel[3];
    if constexpr (VAR == DR_VARIANT_GYM) {
#pragma unroll
        for (int k = F_TGT; k < F_N; ++k) st[k] = *at(fp.p[k], i);
    } else if constexpr (T::MOVING) {
#pragma unroll
        for (int k = 0; k < 3; ++k) cen[k] = *at(fp.p[F_TGT + k], i);
#pragma unroll
        for (int k = 0; k < 9; ++k) mp[k] = *at(v.mot + k * v.stride, i);
    } else {
        st[F_TGT + 0] = (S)0;
        st[F_TGT + 1] = (S)0;
        st[F_TGT + 2] = (S)10.0;
    }
    int32_t step = *at(fp.step, i);
    int32_t ep_num = 0;
    double eps = 0.0;
    if constexpr (T::GYMLIKE) {
        ep_num = *at(fp.ep_num, i);
        eps = *at(fp.eps, i);
    }
    // every state load landed before the loop (else the compiler waits for
    // them at their first uses inside it, as vmcnt(0))
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bool reset_any = false;
    float ob[OD];
    EnvView<S> vk = v;
    // the next reset's Philox blocks drawn ahead, once per group of
    // kResetAhead steps (env_rollout_kernel)
    constexpr int NB = T::NB;
    u32x4 nd[NB] = {};
    bool nd_ok = false;
    int32_t max_steps;
    asm volatile("v_mov_b32 %0, %1" : "=v"(max_steps) : "s"(v.max_steps));
    asm volatile("s_barrier" ::: "memory");                          // B_(-1)
    for (int t = 0; t < K; ++t) {
        asm volatile("" : "+s"(vk.seed_lo), "+s"(vk.seed_hi));
        const float4 a_cur = sh.act[t % kWsNA][p * 64 + lane];
        const MotorMix mx = motor_mix(a_cur);
        if constexpr (T::GYMLIKE) {
            if (t % kResetAhead == 0 && !nd_ok) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    nd[b] = philox4x32_10(u32x4{(uint32_t)(ep_num + 1), (uint32_t)gid,
                                                (uint32_t)(gid >> 32), TAG_RESET | (uint32_t)b},
                                          vk.seed_lo, vk.seed_hi);
                nd_ok = true;
            }
        }
        if constexpr (T::MOVING)
            moving_target(cen, mp, step + 1, (float)v.dt, &st[F_TGT], tvel);
        bool crash;
        S r;
        r = physics_step_mixed<S, VAR>(st, mx, v.dt, crash);
        step += 1;
        const bool done = live && (crash || (step >= max_steps));
        if constexpr (T::GYMLIKE) {
            const bool rs = done && io.auto_reset;
            if (rs) {
                step = 0;
                reset_any = true;
                // a second reset within the group: draw its blocks here (the
                // same words the reset would draw; always passing the array
                // keeps it in registers -- a pointer-or-null argument put it
                // on the scratch stack)
                if (!nd_ok) {
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        nd[b] = philox4x32_10(u32x4{(uint32_t)(ep_num + 1), (uint32_t)gid,
                                                    (uint32_t)(gid >> 32),
                                                    TAG_RESET | (uint32_t)b},
                                              vk.seed_lo, vk.seed_hi);
                }
                if constexpr (VAR == DR_VARIANT_GYM) {
                    gym_reset_regs(vk, i, 0, st, ep_num, eps, &nd[0]);
                } else {
                    moving_reset_regs(vk, i, 0, st, cen, mp, ep_num, eps, nd);
                    moving_target(cen, mp, 0, (float)v.dt, &st[F_TGT], tvel);
                }
                nd_ok = false;
                ep_num += 1;
                if (ep_num % 2000 == 0) eps += 0.1;
            }
        }
        make_obs<S, VAR>(st, ob, tvel);
        if (!live) {
#pragma unroll
            for (int k = 0; k < OD; ++k) ob[k] = 0.f;
        }
        const int so = t & 1;
        float *srow = &sh.obs[so][(p * 64 + lane) * OD];
#pragma unroll
        for (int k = 0; k < OD; ++k) srow[k] = ob[k];
        sh.rew[so][p * 64 + lane] = (float)r;
        sh.done[so][p * 64 + lane] = (uint8_t)done;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_t
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < 12; ++k) st_out(at(fp.p[k], i), st[k]);
        st_out(at(fp.step, i), step);
        if (reset_any) {
            if constexpr (VAR == DR_VARIANT_GYM) {
#pragma unroll
                for (int k = F_TGT; k < F_N; ++k) *at(fp.p[k], i) = st[k];
            } else if constexpr (T::MOVING) {
#pragma unroll
                for (int k = 0; k < 3; ++k) *at(fp.p[F_TGT + k], i) = cen[k];
#pragma unroll
                for (int k = 0; k < 9; ++k) *at(v.mot + k * v.stride, i) = mp[k];
            }
        }
    }
}

// ----------------------------------------------------------------------------
// Split-physics K-step rollout (gym variant, actions read from HBM).  The
// warp-specialised kernel's physics wave, split by DATA into two waves on the
// same SIMD, so that two dependent f64 chains interleave where one wave per
// SIMD left the VALU idle about half of its cycles (two physics waves per
// SIMD were measured to hide 24 % per env):
//   * the TRANSLATION wave (waves 0-3) owns pos / vel / target, the step
//     counter, the curriculum and the reset draws: the yaw's sincos, R's
//     column 2 from the step's Euler sincos, acceleration, velocity,
//     position, reward, crash, done, the reset, and the obs fields pos / vel
//     / target - pos;
//   * the ROTATION wave (waves 4-7) owns the Euler angles and body rates:
//     the roll and pitch sincos, the Euler rates and the angular update, and
//     the obs fields euler / omega;
//   * the MEMORY waves (8-11) load actions and stream outputs as in the
//     warp-specialised kernel.
// Wave p, p + 4 and p + 8 share SIMD p.  The two halves of a step touch
// disjoint state; what crosses is the roll / pitch sincos and the yaw
// (rotation -> translation, formed one step ahead from the updated angles,
// through a double-buffered LDS slot) and the done flag (translation ->
// rotation, read one phase later: a reset zeroes the angles and rates before
// the next step, and their sincos is then exactly (+0, 1), which both waves
// substitute).  The rotation wave therefore writes step t's euler / omega
// obs fields in phase t + 1, and the memory waves store step t's outputs in
// phase t + 2 from three output slots.  Every expression is
// physics_step_mixed's, in its order: outputs bitwise those of the other
// kernels (tests/test_rollout_gpu.py).  Each angle's sincos depends on that
// angle alone, so the yaw's moving waves changes no bit: 41.6-43.3 vs
// 42.6-44.7 us per 32-step launch (round 4, alternating on one box; without
// the rotation wave's sincos altogether, a wrong-result diagnostic build,
// 33.3-34.4 us: that sincos was the launch's critical path).
// ----------------------------------------------------------------------------
// The translation wave stages the squared target distance and the memory
// wave forms the reward from it (the same sqrt and reward arithmetic, off the
// translation wave's instruction stream): 41.3-41.9 vs 43.0-44.2 us per
// 32-step launch against the translation wave forming it (round 3).
constexpr int kAbThreads = 3 * kWsEnvs;   // 4 translation + 4 rotation + 4 memory waves
constexpr int kAbOut = 3;                 // output slots

template <typename S, int OD>
struct AbLds {
    float obs[kAbOut][kWsEnvs * OD];
    S d2[kAbOut][kWsEnvs];                // squared target distance
    uint8_t done[kAbOut][kWsEnvs];
    float4 act[kWsNA][kWsEnvs];
    S sc[2][4][kWsEnvs];                  // sin phi, theta, cos phi, theta
    S psi[2][kWsEnvs];                    // the yaw itself
};

template <typename S>
__global__ __launch_bounds__(kAbThreads) void env_rollout_ab_kernel(EnvView<S> v, RolloutIO io,
                                                                    FieldPtrs<S> fp) {
    constexpr int OD = Traits<DR_VARIANT_GYM>::OD;
    constexpr int NQ = (64 * OD / 4 + 63) / 64;
    constexpr int S_OPS = NQ + 2;
    static_assert(S_OPS + kWsAhead * (S_OPS + 1) <= 63, "the action-load wait count must fit vmcnt");
    __shared__ __attribute__((aligned(16))) AbLds<S, OD> sh;
    const int64_t n_ = v.n;
    const int K = io.k;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = wid & 3;
    const int role = wid >> 2;                    // 0 translation, 1 rotation, 2 memory
    const int ps = p * 64 + lane;                 // this lane's env within the block
    const int64_t wbase = (int64_t)blockIdx.x * kWsEnvs + p * 64;
    const int64_t i_own = wbase + lane;
    const bool live = i_own < n_;
    const int64_t i = live ? i_own : n_ - 1;

    if (role == 2) {
        // ---------------- memory wave (env_rollout_ws_kernel's, stores two
        // phases behind the translation wave, three output slots; actions
        // only from HBM: launch_rollout says why the random policy stays on
        // the warp-specialised kernel).  Kept as its own copy: as one
        // function shared with that kernel it changed this kernel's device
        // code ----------
        const int64_t nvalid = (n_ - wbase) < 64 ? (n_ - wbase) : 64;
        const bool full = nvalid == 64 && (((uintptr_t)io.obs) & 15) == 0 &&
                          ((n_ * OD) & 3) == 0;
        const float4 *acts = reinterpret_cast<const float4 *>(io.actions);
        auto load_act = [&](int t) {
            if (nvalid > 0) {
                ws_glds16(at(acts + (int64_t)t * n_, i),
                          (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)
                              &sh.act[t % kWsNA][p * 64]);
            }
        };
        auto store_out = [&](int t) {
            if (nvalid <= 0) return;
            const int so = t % kAbOut;
            const int64_t row = (int64_t)t * n_;
            const float *src = &sh.obs[so][p * 64 * OD];
            float *dst = io.obs + (row + wbase) * OD;
            // physics_step_mixed's reward (gym variant) from the staged d^2
            const S dd = m_sqrt(sh.d2[so][ps]);
            S rr = (S)0.01 * -dd;
            if (dd < (S)0.05) rr += (S)1;
            const float r = (float)rr;
            const uint8_t d = sh.done[so][ps];
            if (full) {
                float4 q[NQ];
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    if (j * 64 + lane < 64 * OD / 4)
                        q[j] = reinterpret_cast<const float4 *>(src)[j * 64 + lane];
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    if (j * 64 + lane < 64 * OD / 4)
                        st_out(reinterpret_cast<float4 *>(dst) + j * 64 + lane, q[j]);
            } else {
                for (int q = lane; q < (int)nvalid * OD; q += 64) st_out(dst + q, src[q]);
            }
            if (live) {
                st_out(at(io.rew + row, i_own), r);
                st_out(at(io.done + row, i_own), d);
            }
        };
        for (int t = 0; t <= kWsAhead && t < K; ++t) load_act(t);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // actions 0 .. D
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_(-1)
        for (int t = 0; t < K; ++t) {
            if (t + kWsAhead + 1 < K) load_act(t + kWsAhead + 1);
            if (t >= 2) store_out(t - 2);
            // action t + 1 lands before B_t.  Issued in phase q = t - D;
            // younger in the steady state (q >= 2, loads through phase t):
            // q's S_OPS stores and D phases of one load and S_OPS stores;
            // otherwise at least this phase's S_OPS stores (t >= D >= 2).
            if (t + 1 < K && t + 1 > kWsAhead) {
                __builtin_amdgcn_sched_barrier(0);
                if (!full)
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (t >= kWsAhead + 2 && t + kWsAhead + 1 < K)
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S_OPS + kWsAhead * (S_OPS + 1))
                                 : "memory");
                else
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S_OPS) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_t
        }
        asm volatile("s_barrier" ::: "memory");   // B_K: step K - 1's euler / omega staged
        if (K >= 2) store_out(K - 2);
        if (K >= 1) store_out(K - 1);
        return;
    }

    if (role == 1) {
        // ---------------- rotation wave ----------------
        S eul[3], omg[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            eul[k] = *at(fp.p[F_EUL + k], i);
            omg[k] = *at(fp.p[F_OMG + k], i);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        S sn[2], cs[2];
        m_sincos_n<2>(eul, sn, cs);
        sh.psi[0][ps] = eul[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            sh.sc[0][k][ps] = sn[k];
            sh.sc[0][2 + k][ps] = cs[k];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_(-1)
        // the reset of step t - 1 (done flag staged by the translation wave
        // before B_(t-1)) and the obs fields of step t - 1
        auto after_step = [&](int tp) {
            const bool rs = io.auto_reset && sh.done[tp % kAbOut][ps];
            if (rs) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    eul[k] = (S)0;
                    omg[k] = (S)0;
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    sn[k] = (S)0;      // sincos(+0) = (+0, 1) exactly
                    cs[k] = (S)1;
                }
            }
            float *srow = &sh.obs[tp % kAbOut][ps * OD];
#pragma unroll
            for (int k = 0; k < 3; ++k) {     // dead lanes' rows are never stored
                srow[F_EUL + k] = (float)eul[k];
                srow[F_OMG + k] = (float)omg[k];
            }
        };
        for (int t = 0; t < K; ++t) {
            const float4 a_cur = sh.act[t % kWsNA][ps];
            if (t >= 1) after_step(t - 1);
            const MotorMix mx = motor_mix(a_cur);
            // physics_step_mixed's angular part, in its order
            const S tau_phi = (S)kFactor * (S)mx.phi;
            const S tau_theta = (S)kFactor * (S)mx.theta;
            const float tau_psi = kKyaw32 * mx.psi;
            const S sph = sn[0], cph = cs[0], sth = sn[1], cth = cs[1];
            const S w0 = omg[0], w1 = omg[1], w2 = omg[2];
            const S sec = (S)1 / cth;
            const S tth = div_rcp(sth, cth, sec);
            const S ed2 = ((S)0 * w0 + div_rcp(sph, cth, sec) * w1) + div_rcp(cph, cth, sec) * w2;
            const S ed0 = ((S)1 * w0 + (sph * tth) * w1) + (cph * tth) * w2;
            const S ed1 = ((S)0 * w0 + cph * w1) + (-sph) * w2;
            eul[0] += ed0 * v.dt;
            eul[1] += ed1 * v.dt;
            eul[2] += ed2 * v.dt;
            const S wd0 = div_rcp(tau_phi - (S)(kIyy - kIzz) * w1 * w2, (S)kIxx, (S)(1.0 / kIxx));
            const S wd1 = div_rcp(tau_theta - (S)(kIzz - kIxx) * w0 * w2, (S)kIyy, (S)(1.0 / kIyy));
            const S wd2 = div_rcp((S)tau_psi - (S)(kIxx - kIyy) * w0 * w1, (S)kIzz, (S)(1.0 / kIzz));
            omg[0] += wd0 * v.dt;
            omg[1] += wd1 * v.dt;
            omg[2] += wd2 * v.dt;
            // the next step's sincos (of the angles before any reset of this
            // step: the translation wave substitutes (+0, 1) after one)
            m_sincos_n<2>(eul, sn, cs);
            if (t + 1 < K) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    sh.sc[(t + 1) & 1][k][ps] = sn[k];
                    sh.sc[(t + 1) & 1][2 + k][ps] = cs[k];
                }
                sh.psi[(t + 1) & 1][ps] = eul[2];
            }
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_t
        }
        if (K >= 1) after_step(K - 1);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_K
        if (live) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                st_out(at(fp.p[F_EUL + k], i), eul[k]);
                st_out(at(fp.p[F_OMG + k], i), omg[k]);
            }
        }
        return;
    }

    // ---------------- translation wave ----------------
    const uint64_t gid = (uint64_t)(v.env_id_offset + i);
    S st[F_N];                // euler / omega entries unused here
#pragma unroll
    for (int k = 0; k < F_EUL; ++k) st[k] = *at(fp.p[k], i);
#pragma unroll
    for (int k = F_TGT; k < F_N; ++k) st[k] = *at(fp.p[k], i);
#pragma unroll
    for (int k = F_EUL; k < F_TGT; ++k) st[k] = (S)0;
    int32_t step = *at(fp.step, i);
    int32_t ep_num = *at(fp.ep_num, i);
    double eps = *at(fp.eps, i);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bool reset_any = false, prev_rs = false;
    EnvView<S> vk = v;
    // the next reset's state, prepared when its Philox block is drawn (once
    // per group of kResetAhead steps for the lanes whose draw was used)
    GymNext<S> nx = {};
    bool nd_ok = false;
    int32_t max_steps;
    asm volatile("v_mov_b32 %0, %1" : "=v"(max_steps) : "s"(v.max_steps));
    auto draw_next = [&]() {
        const u32x4 r0 = philox4x32_10(u32x4{(uint32_t)(ep_num + 1), (uint32_t)gid,
                                             (uint32_t)(gid >> 32), TAG_RESET},
                                       vk.seed_lo, vk.seed_hi);
        nx = gym_next_reset(vk, gid, ep_num, eps, r0);
    };
    asm volatile("s_barrier" ::: "memory");                          // B_(-1)
    for (int t = 0; t < K; ++t) {
        asm volatile("" : "+s"(vk.seed_lo), "+s"(vk.seed_hi));
        const float4 a_cur = sh.act[t % kWsNA][ps];
        // the yaw's sincos here (only R's column 2 needs it), the roll and
        // pitch's from the rotation wave
        S sn[3], cs[3];
        const S psi = sh.psi[t & 1][ps];
        m_sincos_n<1>(&psi, &sn[2], &cs[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sn[k] = prev_rs ? (S)0 : (k < 2 ? sh.sc[t & 1][k][ps] : sn[k]);
            cs[k] = prev_rs ? (S)1 : (k < 2 ? sh.sc[t & 1][2 + k][ps] : cs[k]);
        }
        const MotorMix mx = motor_mix(a_cur);
        if (t % kResetAhead == 0 && !nd_ok) {
            draw_next();
            nd_ok = true;
        }
        // physics_step_mixed's translational part, in its order
        const float thr = mx.thr;
        const S sph = sn[0], cph = cs[0], sth = sn[1], cth = cs[1], sps = sn[2], cps = cs[2];
        const S r02 = cps * sth * cph + sps * sph;
        const S r12 = sps * sth * cph - cps * sph;
        const S r22 = cth * cph;
        const S T = (S)thr;
        const S acc0 = (S)0 + (r02 * T) / (S)kMass;
        const S acc1 = (S)0 + (r12 * T) / (S)kMass;
        const S acc2 = (S)(-kG) + (r22 * T) / (S)kMass;
        st[F_VEL + 0] += acc0 * v.dt;
        st[F_VEL + 1] += acc1 * v.dt;
        st[F_VEL + 2] += acc2 * v.dt;
#pragma unroll
        for (int k = 0; k < 3; ++k) st[F_POS + k] += st[F_VEL + k] * v.dt;
        const S dx = st[F_POS + 0] - st[F_TGT + 0];
        const S dy = st[F_POS + 1] - st[F_TGT + 1];
        const S dz = st[F_POS + 2] - st[F_TGT + 2];
        const S dist2 = (dx * dx + dy * dy) + dz * dz;
        const S px = st[F_POS + 0], py = st[F_POS + 1], pz = st[F_POS + 2];
        const S pn2 = (px * px + py * py) + pz * pz;
        const bool crash = (pz < (S)0) || (pn2 > (S)2500);
        step += 1;
        const bool done = live && (crash || (step >= max_steps));
        const bool rs = done && io.auto_reset;
        const int so = t % kAbOut;
        // staged before the reset: the squared distance is of the pre-reset
        // position (otherwise the compiler sinks it below the reset branch and
        // keeps both states live, with a copy of each per step)
        sh.d2[so][ps] = dist2;
        sh.done[so][ps] = (uint8_t)done;
        if (rs) {
            // gym_reset_regs on the prepared state (a second reset within
            // the group draws here, as the reset itself would)
            step = 0;
            reset_any = true;
            if (!nd_ok) draw_next();
            ep_num += 1;
            vk.ep_num[i] = ep_num;
            eps = nx.eps;
            if (nx.bump) vk.eps[i] = eps;
            st[F_POS + 0] = nx.px;
            st[F_POS + 1] = nx.py;
            st[F_POS + 2] = (S)1.0;
#pragma unroll
            for (int k = F_VEL; k < F_VEL + 3; ++k) st[k] = (S)0;
            st[F_TGT + 0] = nx.tx;
            st[F_TGT + 1] = nx.ty;
            st[F_TGT + 2] = nx.tz;
            nd_ok = false;
        }
        prev_rs = rs;
        float *srow = &sh.obs[so][ps * OD];
        // a dead lane's (i >= n) row is staged but never stored (the memory
        // wave stores the live rows only), so it needs no zeroing
#pragma unroll
        for (int k = 0; k < F_EUL; ++k) srow[k] = (float)st[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) srow[12 + k] = (float)(st[F_TGT + k] - st[F_POS + k]);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // B_t
    }
    asm volatile("s_barrier" ::: "memory");                          // B_K
    if (live) {
#pragma unroll
        for (int k = 0; k < F_EUL; ++k) st_out(at(fp.p[k], i), st[k]);
        st_out(at(fp.step, i), step);
        if (reset_any) {
#pragma unroll
            for (int k = F_TGT; k < F_N; ++k) *at(fp.p[k], i) = st[k];
        }
    }
}


// Reset (all envs, or those with mask[i] != 0) and write every env's obs.
// mode: 0 Philox, 1 host uniforms, 2 constant 0.5.  `init` additionally
// clears ep_num / eps / monitor counters first (constructor).
template <typename S, int VAR>
__global__ __launch_bounds__(kBlock) void env_reset_kernel(EnvView<S> v,
                                                           const uint8_t *mask,
                                                           float *obs, int mode,
                                                           int init) {
    constexpr int OD = Traits<VAR>::OD;
    __shared__ float4 sh4[kBlock * OD / 4];
    const int64_t base = (int64_t)blockIdx.x * kBlock;
    const int64_t i = base + threadIdx.x;
    float ob[OD];
    if constexpr (VAR == DR_VARIANT_TAG) {
        // Each drone resets as the gym's does; a pair resets if either
        // member's mask byte is set (n is even: i ^ 1 < n).  The partner's
        // fresh state comes from a lane exchange outside the `in` branch,
        // never from memory another lane writes in this launch.
        const bool in = i < v.n;
        S st[F_N] = {};
        if (in) {
            if (init) {
                v.ep_num[i] = 0;
                v.eps[i] = 0.0;
                v.ep_ret[i] = 0.f;
                v.ep_len[i] = 0;
            }
            if ((mask == nullptr) || mask[i] || mask[i ^ 1]) {
                gym_reset_regs(v, i, mode, st, v.ep_num[i], v.eps[i]);
#pragma unroll
                for (int k = 0; k < F_N; ++k) v.field(k)[i] = st[k];
                v.step[i] = 0;
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) st[k] = v.field(k)[i];
            }
        }
        S pp[3], pv[3];
        float tx[7];
        tag_partner(st, pp, pv);
        tag_ext(st, pp, pv, (i & 1) == 0 ? 1.0f : -1.0f, tx);
        make_obs<S, VAR>(st, ob, tx);
        if (!in) {
#pragma unroll
            for (int k = 0; k < OD; ++k) ob[k] = 0.f;
        }
    } else if (i < v.n) {
        if (init) {
            v.ep_num[i] = 0;
            v.eps[i] = 0.0;
            v.ep_ret[i] = 0.f;
            v.ep_len[i] = 0;
        }
        S st[F_N];
        float tvel[3] = {0.f, 0.f, 0.f};
        S qd = (S)0;              // rk4: the quaternion's fourth word
        const bool doit = (mask == nullptr) || mask[i];
        if (doit) {
            if constexpr (VAR == DR_VARIANT_GYM) {
                gym_reset_regs(v, i, mode, st, v.ep_num[i], v.eps[i]);
            } else if constexpr (VAR == DR_VARIANT_RK4) {
                gym_reset_regs(v, i, mode, st, v.ep_num[i], v.eps[i]);
                rk4_reset_quat(st, qd);
                reinterpret_cast<S *>(v.mot)[i] = qd;
            } else if constexpr (VAR == DR_VARIANT_SMOOTH) {
                gym_reset_regs(v, i, mode, st, v.ep_num[i], v.eps[i]);
#pragma unroll
                for (int k = 0; k < 4; ++k) v.mot[k * v.stride + i] = kHover32;
            } else if constexpr (VAR == DR_VARIANT_MOVING) {
                float mp[9];
                moving_reset_regs(v, i, mode, st, &st[F_TGT], mp, v.ep_num[i], v.eps[i]);
#pragma unroll
                for (int k = 0; k < 9; ++k) v.mot[k * v.stride + i] = mp[k];
            } else {
                vec_reset_regs(st);
            }
#pragma unroll
            for (int k = 0; k < F_N; ++k) v.field(k)[i] = st[k];
            v.step[i] = 0;
        } else {
#pragma unroll
            for (int k = 0; k < F_N; ++k) st[k] = v.field(k)[i];
            if constexpr (VAR == DR_VARIANT_RK4) qd = reinterpret_cast<S *>(v.mot)[i];
        }
        if constexpr (VAR == DR_VARIANT_MOVING) {
            // stored target = the centre; the obs sees the target at `step`
            S cen[3] = {st[F_TGT], st[F_TGT + 1], st[F_TGT + 2]};
            float mp[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) mp[k] = v.mot[k * v.stride + i];
            moving_target(cen, mp, v.step[i], (float)v.dt, &st[F_TGT], tvel);
        }
        if constexpr (VAR == DR_VARIANT_SMOOTH) {
            float fm[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) fm[k] = v.mot[k * v.stride + i];
            make_obs<S, VAR>(st, ob, fm);
        } else if constexpr (VAR == DR_VARIANT_RK4) {
            const float qx[1] = {(float)qd};
            make_obs<S, VAR>(st, ob, qx);
        } else {
            make_obs<S, VAR>(st, ob, tvel);
        }
    } else {
#pragma unroll
        for (int k = 0; k < OD; ++k) ob[k] = 0.f;
    }
    if (obs) store_obs_block<OD>(reinterpret_cast<float *>(sh4), ob, obs, base, v.n);
}

template <typename S>
__global__ void get_field_kernel(EnvView<S> v, int field, void *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n) return;
    if (field <= DR_FIELD_TARGET) {
        double *o = static_cast<double *>(out);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[i * 3 + k] = (double)v.field(field * 3 + k)[i];
    } else if (field == DR_FIELD_STEP) {
        static_cast<int32_t *>(out)[i] = v.step[i];
    } else if (field == DR_FIELD_EP_NUM) {
        static_cast<int32_t *>(out)[i] = v.ep_num[i];
    } else if (field == DR_FIELD_EPS) {
        static_cast<double *>(out)[i] = v.eps[i];
    } else if (field == DR_FIELD_EP_RETURN) {
        static_cast<float *>(out)[i] = v.ep_ret[i];
    } else if (field == DR_FIELD_EP_LENGTH) {
        static_cast<int32_t *>(out)[i] = v.ep_len[i];
    } else if (field == DR_FIELD_MOTION) {
#pragma unroll
        for (int k = 0; k < 9; ++k) static_cast<float *>(out)[i * 9 + k] = v.mot[k * v.stride + i];
    }
}

template <typename S>
__global__ void gather_field_kernel(EnvView<S> v, int field, const int32_t *ids, int64_t k,
                                    void *out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const int64_t i = ids[j];
    if (i < 0 || i >= v.n) return;
    if (field <= DR_FIELD_TARGET) {
        double *o = static_cast<double *>(out);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[j * 3 + c] = (double)v.field(field * 3 + c)[i];
    } else if (field == DR_FIELD_STEP) {
        static_cast<int32_t *>(out)[j] = v.step[i];
    } else if (field == DR_FIELD_EP_NUM) {
        static_cast<int32_t *>(out)[j] = v.ep_num[i];
    } else if (field == DR_FIELD_EPS) {
        static_cast<double *>(out)[j] = v.eps[i];
    } else if (field == DR_FIELD_EP_RETURN) {
        static_cast<float *>(out)[j] = v.ep_ret[i];
    } else if (field == DR_FIELD_EP_LENGTH) {
        static_cast<int32_t *>(out)[j] = v.ep_len[i];
    } else if (field == DR_FIELD_MOTION) {
#pragma unroll
        for (int c = 0; c < 9; ++c) static_cast<float *>(out)[j * 9 + c] = v.mot[c * v.stride + i];
    }
}

template <typename S>
__global__ void set_field_kernel(EnvView<S> v, int field, const void *in) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n) return;
    if (field <= DR_FIELD_TARGET) {
        const double *p = static_cast<const double *>(in);
#pragma unroll
        for (int k = 0; k < 3; ++k) v.field(field * 3 + k)[i] = (S)p[i * 3 + k];
    } else if (field == DR_FIELD_STEP) {
        v.step[i] = static_cast<const int32_t *>(in)[i];
    } else if (field == DR_FIELD_EP_NUM) {
        v.ep_num[i] = static_cast<const int32_t *>(in)[i];
    } else if (field == DR_FIELD_EPS) {
        v.eps[i] = static_cast<const double *>(in)[i];
    } else if (field == DR_FIELD_EP_RETURN) {
        v.ep_ret[i] = static_cast<const float *>(in)[i];
    } else if (field == DR_FIELD_EP_LENGTH) {
        v.ep_len[i] = static_cast<const int32_t *>(in)[i];
    } else if (field == DR_FIELD_MOTION) {
#pragma unroll
        for (int k = 0; k < 9; ++k) v.mot[k * v.stride + i] = static_cast<const float *>(in)[i * 9 + k];
    }
}

// DR_FIELD_MOTOR (smooth variant), a kernel of its own so the field kernels
// above stay as they were: row j of the (k,4) f32 buffer `io` is read from
// (get: ids null, env j; gather: env ids[j]) or written to (set) the 4 motor
// arrays at `mot`.
__global__ void motor_field_kernel(float *mot, int64_t stride, int64_t n, const int32_t *ids,
                                   int64_t k, float *io, int set) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const int64_t i = ids ? (int64_t)ids[j] : j;
    if (i < 0 || i >= n) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (set) mot[c * stride + i] = io[j * 4 + c];
        else io[j * 4 + c] = mot[c * stride + i];
    }
}

// DR_FIELD_QUAT (rk4 variant), a kernel of its own like DR_FIELD_MOTOR's:
// row j of the (k,4) buffer `io`, in the state scalar, is read from (get: ids
// null, env j; gather: env ids[j]) or written to (set) the attitude (w, x,
// y, z): the three arrays at F_EUL and the one at `mot`.
template <typename S>
__global__ void quat_field_kernel(EnvView<S> v, const int32_t *ids, int64_t k, S *io, int set) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const int64_t i = ids ? (int64_t)ids[j] : j;
    if (i < 0 || i >= v.n) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        S *p = (c < 3 ? v.field(F_EUL + c) : reinterpret_cast<S *>(v.mot)) + i;
        if (set) *p = io[j * 4 + c];
        else io[j * 4 + c] = *p;
    }
}

// Wind: the mean wind of each env's CURRENT episode (ep_num as stored) and a
// zero gust, for every env (mask null: the enabling dr_set_wind, dr_reset) or
// those with mask[i] != 0 (dr_reset_masked).  Runs behind the gym's
// env_reset_kernel on the same stream, which has already counted the new
// episode, so that kernel and its argument block stay the gym's.
__global__ __launch_bounds__(kBlock) void wind_fill_kernel(float *wind, int64_t stride, int64_t n,
                                                           const int32_t *ep_num,
                                                           int64_t env_id_offset, uint32_t k0,
                                                           uint32_t k1, float W,
                                                           const uint8_t *mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    float m[3];
    wind_mean(k0, k1, (uint64_t)(env_id_offset + i), ep_num[i], W, m);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        wind[k * stride + i] = m[k];
        wind[(3 + k) * stride + i] = 0.f;
    }
}

// DR_FIELD_WIND, as motor_field_kernel: row j of the (k,6) f32 buffer `io`
// (mean wind xyz, gust xyz) is read from or written to the six wind arrays.
__global__ void wind_field_kernel(float *wind, int64_t stride, int64_t n, const int32_t *ids,
                                  int64_t k, float *io, int set) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const int64_t i = ids ? (int64_t)ids[j] : j;
    if (i < 0 || i >= n) return;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        if (set) wind[c * stride + i] = io[j * 6 + c];
        else io[j * 6 + c] = wind[c * stride + i];
    }
}

// Airframe: the six words of each env's CURRENT episode (ep_num as stored),
// for every env (mask null: the enabling dr_set_airframe, dr_reset) or those
// with mask[i] != 0 (dr_reset_masked).  Runs behind the gym's env_reset_kernel
// on the same stream, as wind_fill_kernel does.
__global__ __launch_bounds__(kBlock) void airframe_fill_kernel(
    float *air, int64_t stride, int64_t n, const int32_t *ep_num, int64_t env_id_offset,
    uint32_t k0, uint32_t k1, VarArgs<KVAR_AIRFRAME> va, const uint8_t *mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    float af[6];
    airframe_draw(k0, k1, (uint64_t)(env_id_offset + i), ep_num[i], va, af);
#pragma unroll
    for (int k = 0; k < 6; ++k) air[k * stride + i] = af[k];
}

// Waypoints: a new course (j = 0) for every env (mask null: dr_reset) or those
// with mask[i] != 0 (dr_reset_masked); the reach counter q stays.  Runs behind
// the gym's env_reset_kernel on the same stream, as wind_fill_kernel does.
__global__ __launch_bounds__(kBlock) void waypoint_restart_kernel(int32_t *wp, int64_t n,
                                                                  const uint8_t *mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) return;
    wp[i] = 0;
}

// DR_FIELD_WAYPOINT, as wind_field_kernel: row j of the (k,2) i32 buffer `io`
// (index within the episode, reaches since enabling).
__global__ void waypoint_field_kernel(int32_t *wp, int64_t stride, int64_t n, const int32_t *ids,
                                      int64_t k, int32_t *io, int set) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const int64_t i = ids ? (int64_t)ids[j] : j;
    if (i < 0 || i >= n) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (set) wp[c * stride + i] = io[j * 2 + c];
        else io[j * 2 + c] = wp[c * stride + i];
    }
}

__global__ __launch_bounds__(kBlock) void random_actions_kernel(
    int64_t n, uint32_t k0, uint32_t k1, int64_t env_off, uint64_t step,
    float lo, float span, float4 *out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t gid = (uint64_t)(env_off + i);
    out[i] = action_of(step, gid, k0, k1, lo, span);
}

}  // namespace
}  // namespace dr

// ============================================================================
// C ABI
// ============================================================================
using namespace dr;

struct dr_handle {
    dr_config cfg{};
    int64_t n = 0;
    int64_t stride = 0;
    int obs_dim = 15;
    // envs per wave of env_step_kernel: 64, or 32 (half-populated waves:
    // twice the waves in flight); chosen by batch size in dr_create
    int rpw = 64;
    bool nt_loads = false;  // nontemporal state loads (large batches)
    // DR_VARIANT_SMOOTH (dr_set_smoothing): passed to each launch
    float alpha = 1.0f;
    float rate_penalty = 0.0f;
    // DR_VARIANT_TAG (dr_set_tag): passed to each launch
    float tag_radius = 0.25f;
    float crash_penalty = 0.0f;
    // DR_VARIANT_GYM, its options (dr_set_wind, dr_set_waypoints,
    // dr_set_airframe).  At most one is enabled: `opt_kind` says which, and
    // `opt` is its allocation of `stride`-element arrays (wind: 6 f32, mean
    // and gust; waypoints: 2 i32, j and q; airframe: 6 f32, m, s, g0..g3),
    // made by the first enabling call; while OPT_NONE the handle launches the
    // gym's kernels.  The parameters are kept as given and passed to each
    // launch; gust_b = 1 - gust_rate and gust_c = sigma sqrt(3 (1 - b^2)) are
    // the two the host derives.
    enum Opt : int { OPT_NONE = 0, OPT_WIND, OPT_WAYPOINT, OPT_AIRFRAME };
    int opt_kind = OPT_NONE;
    void *opt = nullptr;
    float drag = 0.0f, wind_speed = 0.0f, gust_sigma = 0.0f, gust_rate = 0.0f;
    float gust_b = 1.0f, gust_c = 0.0f;
    float reach_radius = 0.0f, reach_bonus = 0.0f;
    float mass_spread = 0.0f, inertia_spread = 0.0f, motor_spread = 0.0f;
    void *mem = nullptr;
    const double *host_u = nullptr;
    std::string err;
};

namespace dr {
static thread_local std::string g_err;
void set_global_error(const std::string &msg) { g_err = msg; }
const char *global_error() { return g_err.c_str(); }
}  // namespace dr

namespace {

int fail(dr_handle *h, int code, const std::string &msg) {
    if (h)
        h->err = msg;
    else
        set_global_error(msg);
    return code;
}

// The epilogue of every kernel launch: `what` prefixes the HIP error's text.
int launched(dr_handle *h, const std::string &what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, DR_ERR_HIP, what + ": " + hipGetErrorString(e));
    return DR_OK;
}

// f(std::integral_constant<int, V>{}) for a variant id (a public dr_variant or
// one of this file's KVAR_ tags) as a compile-time value: the one list of
// variant ids on the host; what differs between them comes from Traits<V>.
template <typename F>
auto for_variant(int variant, F &&f) {
    switch (variant) {
        case DR_VARIANT_GYM: return f(std::integral_constant<int, DR_VARIANT_GYM>{});
        case KVAR_WIND: return f(std::integral_constant<int, KVAR_WIND>{});
        case KVAR_WAYPOINT: return f(std::integral_constant<int, KVAR_WAYPOINT>{});
        case KVAR_AIRFRAME: return f(std::integral_constant<int, KVAR_AIRFRAME>{});
        case DR_VARIANT_MOVING: return f(std::integral_constant<int, DR_VARIANT_MOVING>{});
        case DR_VARIANT_SMOOTH: return f(std::integral_constant<int, DR_VARIANT_SMOOTH>{});
        case DR_VARIANT_TAG: return f(std::integral_constant<int, DR_VARIANT_TAG>{});
        case DR_VARIANT_RK4: return f(std::integral_constant<int, DR_VARIANT_RK4>{});
        default: return f(std::integral_constant<int, DR_VARIANT_VECTORIZED>{});
    }
}
// bytes per env behind the monitor counters
template <typename S>
size_t mot_bytes(int variant) {
    return for_variant(variant, [](auto var) {
        return Traits<decltype(var)::value>::template mot_bytes<S>();
    });
}

template <typename S>
EnvView<S> view_of(const dr_handle *h) {
    EnvView<S> v{};
    char *m = static_cast<char *>(h->mem);
    const int64_t sp = h->stride;
    v.f = reinterpret_cast<S *>(m);
    v.stride = sp;
    v.eps = reinterpret_cast<double *>(m + Layout<S>::eps(sp));
    v.step = reinterpret_cast<int32_t *>(m + Layout<S>::step(sp));
    v.ep_num = reinterpret_cast<int32_t *>(m + Layout<S>::ep_num(sp));
    v.ep_ret = reinterpret_cast<float *>(m + Layout<S>::ep_ret(sp));
    v.ep_len = reinterpret_cast<int32_t *>(m + Layout<S>::ep_len(sp));
    // the variant's own arrays behind the counters, else (gym) the enabled
    // option's allocation, else null
    v.mot = mot_bytes<S>(h->cfg.variant) ? reinterpret_cast<float *>(m + Layout<S>::mot(sp))
                                         : static_cast<float *>(h->opt);
    v.n = h->n;
    v.env_id_offset = h->cfg.env_id_offset;
    v.host_u = h->host_u;
    v.seed_lo = (uint32_t)h->cfg.seed;
    v.seed_hi = (uint32_t)(h->cfg.seed >> 32);
    v.max_steps = h->cfg.max_steps;
    v.dt = (S)h->cfg.dt;
    return v;
}

size_t state_bytes(int64_t stride, int dtype, int variant) {
    const bool f64 = dtype == DR_STATE_F64;
    const size_t s = f64 ? sizeof(double) : sizeof(float);
    const size_t mot = f64 ? mot_bytes<double>(variant) : mot_bytes<float>(variant);
    return (size_t)F_N * stride * s + (size_t)stride * (8 + 4 + 4 + 4 + 4 + mot);
}

template <typename S>
FieldPtrs<S> field_ptrs_of(const EnvView<S> &v) {
    FieldPtrs<S> fp;
    for (int k = 0; k < F_N; ++k) fp.p[k] = v.field(k);
    fp.step = v.step;
    fp.ep_num = v.ep_num;
    fp.eps = v.eps;
    return fp;
}

inline hipStream_t as_stream(void *s) { return static_cast<hipStream_t>(s); }

// The handle's state scalar and variant as compile-time values:
// f(TypeTag<S>{}, std::integral_constant<int, VAR>{}) for the handle's pair.
template <typename T>
struct TypeTag {
    using type = T;
};
template <typename F>
int with_state(const dr_handle *h, F &&f) {
    // a gym handle with an option enabled launches that option's kernels
    static constexpr int kOptVar[] = {DR_VARIANT_GYM, KVAR_WIND, KVAR_WAYPOINT, KVAR_AIRFRAME};
    const int kv = h->cfg.variant == DR_VARIANT_GYM ? kOptVar[h->opt_kind] : h->cfg.variant;
    auto by_variant = [&](auto s) { return for_variant(kv, [&](auto var) { return f(s, var); }); };
    return h->cfg.state_dtype == DR_STATE_F64 ? by_variant(TypeTag<double>{})
                                              : by_variant(TypeTag<float>{});
}

// The variant's trailing kernel argument (empty but for the smooth and tag
// variants).
template <int VAR>
VarArgs<VAR> var_args(const dr_handle *h) {
    if constexpr (VAR == DR_VARIANT_SMOOTH) return VarArgs<VAR>{h->alpha, h->rate_penalty};
    else if constexpr (VAR == DR_VARIANT_TAG) return VarArgs<VAR>{h->tag_radius, h->crash_penalty};
    else if constexpr (VAR == DR_VARIANT_RK4)
        return VarArgs<VAR>{h->cfg.dt / 6.0, (float)h->cfg.dt / 6.0f};
    else if constexpr (VAR == KVAR_WIND)
        return VarArgs<VAR>{h->drag, h->gust_b, h->gust_c, h->wind_speed};
    else if constexpr (VAR == KVAR_WAYPOINT) return VarArgs<VAR>{h->reach_radius, h->reach_bonus};
    else if constexpr (VAR == KVAR_AIRFRAME)
        return VarArgs<VAR>{h->mass_spread, h->inertia_spread, h->motor_spread};
    else return VarArgs<VAR>{};
}

template <typename S, int VAR>
int launch_reset(dr_handle *h, const uint8_t *mask, float *obs, int mode,
                 int init, hipStream_t st) {
    EnvView<S> v = view_of<S>(h);
    hipLaunchKernelGGL((env_reset_kernel<S, VAR>), dim3(grid_for(h->n)),
                       dim3(kBlock), 0, st, v, mask, obs, mode, init);
    return launched(h, "env_reset_kernel");
}

// The enabled option's words for every env's (mask: the masked envs')
// current episode, enqueued on `st` behind the gym's reset: the mean wind and
// a zero gust; a new course (j = 0); the episode's airframe.
int launch_option_fill(dr_handle *h, const uint8_t *mask, hipStream_t st) {
    const int32_t *ep_num = h->cfg.state_dtype == DR_STATE_F64 ? view_of<double>(h).ep_num
                                                               : view_of<float>(h).ep_num;
    const dim3 grid(grid_for(h->n)), block(kBlock);
    const uint32_t k0 = (uint32_t)h->cfg.seed, k1 = (uint32_t)(h->cfg.seed >> 32);
    switch (h->opt_kind) {
        case dr_handle::OPT_WIND:
            hipLaunchKernelGGL(wind_fill_kernel, grid, block, 0, st, static_cast<float *>(h->opt),
                               h->stride, h->n, ep_num, h->cfg.env_id_offset, k0, k1,
                               h->wind_speed, mask);
            return launched(h, "wind_fill_kernel");
        case dr_handle::OPT_AIRFRAME:
            hipLaunchKernelGGL(airframe_fill_kernel, grid, block, 0, st,
                               static_cast<float *>(h->opt), h->stride, h->n, ep_num,
                               h->cfg.env_id_offset, k0, k1, var_args<KVAR_AIRFRAME>(h), mask);
            return launched(h, "airframe_fill_kernel");
        case dr_handle::OPT_WAYPOINT:
            hipLaunchKernelGGL(waypoint_restart_kernel, grid, block, 0, st,
                               static_cast<int32_t *>(h->opt), h->n, mask);
            return launched(h, "waypoint_restart_kernel");
        default: return DR_OK;
    }
}

int dispatch_reset(dr_handle *h, const uint8_t *mask, float *obs, int mode,
                   int init, hipStream_t st) {
    return with_state(h, [&](auto s, auto var) {
        // an option's handle resets as the gym does (its words are not
        // observed), then fills the new episodes' words behind it
        using T = Traits<decltype(var)::value>;
        int rc = launch_reset<typename decltype(s)::type, T::RESET_VAR>(h, mask, obs, mode, init,
                                                                        st);
        if (T::OPTION && rc == DR_OK) rc = launch_option_fill(h, mask, st);
        return rc;
    });
}

template <typename S, int VAR, bool MON>
int launch_step(dr_handle *h, const StepIO &io, hipStream_t st) {
    EnvView<S> v = view_of<S>(h);
    const FieldPtrs<S> fp = field_ptrs_of(v);
    const VarArgs<VAR> va = var_args<VAR>(h);
    if (Traits<VAR>::GYMLIKE && v.host_u) {   // parity mode
        if (h->rpw == 32)
            hipLaunchKernelGGL((env_step_kernel<S, VAR, MON, 32, true, false>),
                               dim3(grid_for(h->n, kEnvWpb * 32)), dim3(kEnvBlock), 0, st,
                               v, io, fp, va);
        else
            hipLaunchKernelGGL((env_step_kernel<S, VAR, MON, 64, true, false>),
                               dim3(grid_for(h->n, kEnvWpb * 64)), dim3(kEnvBlock), 0, st,
                               v, io, fp, va);
    } else {
        const dim3 g64(grid_for(h->n, kEnvWpb * 64)), g32(grid_for(h->n, kEnvWpb * 32));
        switch (h->rpw * 2 + (int)h->nt_loads) {
            case 64:
                hipLaunchKernelGGL((env_step_kernel<S, VAR, MON, 32, false, false>), g32,
                                   dim3(kEnvBlock), 0, st, v, io, fp, va);
                break;
            case 65:
                hipLaunchKernelGGL((env_step_kernel<S, VAR, MON, 32, false, true>), g32,
                                   dim3(kEnvBlock), 0, st, v, io, fp, va);
                break;
            case 129:
                hipLaunchKernelGGL((env_step_kernel<S, VAR, MON, 64, false, true>), g64,
                                   dim3(kEnvBlock), 0, st, v, io, fp, va);
                break;
            default:
                hipLaunchKernelGGL((env_step_kernel<S, VAR, MON, 64, false, false>), g64,
                                   dim3(kEnvBlock), 0, st, v, io, fp, va);
        }
    }
    return launched(h, "env_step_kernel");
}

template <bool MON>
int dispatch_step(dr_handle *h, const StepIO &io, hipStream_t st) {
    return with_state(h, [&](auto s, auto var) {
        return launch_step<typename decltype(s)::type, decltype(var)::value, MON>(h, io, st);
    });
}

template <typename S, int VAR, bool GEN>
int launch_rollout(dr_handle *h, const RolloutIO &io, hipStream_t st, hipEvent_t e0,
                   hipEvent_t e1) {
    EnvView<S> v = view_of<S>(h);
    const FieldPtrs<S> fp = field_ptrs_of(v);
    // The warp-specialised form while its grid is at most one block per CU
    // (n <= 256 x CUs: 65,536 envs on MI355X), where one physics wave per
    // SIMD has nothing else to overlap with; above that the one-role kernel
    // already runs two or more waves per SIMD, and the warp-specialised one
    // measured equal (gym, 131,072 / 1,048,576 envs) or slower (in-kernel
    // policy at 2^20; the moving variant, whose 175 VGPRs fit one 512-thread
    // block per CU).  DRONERL_ROLLOUT_WS=0 / 1 forces either (A/B).
    static const int ws_env = [] {
        const char *r = std::getenv("DRONERL_ROLLOUT_WS");
        return r ? (std::atoi(r) != 0 ? 1 : 0) : -1;
    }();
    // Traits::ONE_ROLE variants have the one-role kernel only, whatever the
    // override says.
    constexpr bool ONE_ROLE = Traits<VAR>::ONE_ROLE;
    const bool ws = ONE_ROLE
                        ? false
                        : (ws_env >= 0 ? ws_env == 1
                                       : h->n <= (int64_t)kWsEnvs * device_cu_count());
    // with events: hipExtLaunchKernelGGL binds them to the dispatch packet's
    // own start / end timestamps (no extra packets in the queue)
    if (ws) {
        if constexpr (ONE_ROLE) {
            // unreachable: ws is false for these variants
        } else if constexpr (VAR == DR_VARIANT_GYM && !GEN) {
            // the split-physics form of the warp-specialised kernel (gym
            // variant, actions read from HBM; with the in-kernel policy its
            // memory waves' Philox draws share the SIMD with two physics
            // waves and it measured slower, so GEN keeps the one-physics-wave
            // form)
            const dim3 grid(grid_for(h->n, kWsEnvs)), block(kAbThreads);
            if (e0 || e1)
                hipExtLaunchKernelGGL((env_rollout_ab_kernel<S>), grid, block, 0, st, e0, e1, 0,
                                      v, io, fp);
            else
                hipLaunchKernelGGL((env_rollout_ab_kernel<S>), grid, block, 0, st, v, io, fp);
        } else {
            const dim3 grid(grid_for(h->n, kWsEnvs)), block(kWsThreads);
            if (e0 || e1)
                hipExtLaunchKernelGGL((env_rollout_ws_kernel<S, VAR, GEN>), grid, block, 0, st,
                                      e0, e1, 0, v, io, fp);
            else
                hipLaunchKernelGGL((env_rollout_ws_kernel<S, VAR, GEN>), grid, block, 0, st, v,
                                   io, fp);
        }
    } else {
        const dim3 grid(grid_for(h->n, kEnvWpb * 64)), block(kEnvBlock);
        if (e0 || e1)
            hipExtLaunchKernelGGL((env_rollout_kernel<S, VAR, 64, GEN>), grid, block, 0, st, e0,
                                  e1, 0, v, io, fp, var_args<VAR>(h));
        else
            hipLaunchKernelGGL((env_rollout_kernel<S, VAR, 64, GEN>), grid, block, 0, st, v, io,
                               fp, var_args<VAR>(h));
    }
    return launched(h, "env_rollout_kernel");
}

template <bool GEN>
int dispatch_rollout(dr_handle *h, const RolloutIO &io, hipStream_t st, hipEvent_t e0,
                     hipEvent_t e1) {
    return with_state(h, [&](auto s, auto var) {
        return launch_rollout<typename decltype(s)::type, decltype(var)::value, GEN>(h, io, st, e0,
                                                                                     e1);
    });
}

// DR_FIELD_MOTOR of dr_get_state / dr_gather_state / dr_set_state.
int motor_field(dr_handle *h, const char *who, const int32_t *ids, int64_t k, float *io,
                int set, void *stream) {
    if (h->cfg.variant != DR_VARIANT_SMOOTH)
        return fail(h, DR_ERR_INVALID,
                    std::string(who) + ": motor exists only for DR_VARIANT_SMOOTH");
    if (k == 0) return DR_OK;
    DeviceGuard g(h->cfg.device);
    float *mot = h->cfg.state_dtype == DR_STATE_F64 ? view_of<double>(h).mot
                                                    : view_of<float>(h).mot;
    hipLaunchKernelGGL(motor_field_kernel, dim3(grid_for(k)), dim3(kBlock), 0, as_stream(stream),
                       mot, h->stride, h->n, ids, k, io, set);
    return launched(h, who);
}

// DR_FIELD_QUAT of dr_get_state / dr_gather_state / dr_set_state.
int quat_field(dr_handle *h, const char *who, const int32_t *ids, int64_t k, void *io, int set,
               void *stream) {
    if (h->cfg.variant != DR_VARIANT_RK4)
        return fail(h, DR_ERR_INVALID, std::string(who) + ": quat exists only for DR_VARIANT_RK4");
    if (k == 0) return DR_OK;
    DeviceGuard g(h->cfg.device);
    if (h->cfg.state_dtype == DR_STATE_F64)
        hipLaunchKernelGGL(quat_field_kernel<double>, dim3(grid_for(k)), dim3(kBlock), 0,
                           as_stream(stream), view_of<double>(h), ids, k,
                           static_cast<double *>(io), set);
    else
        hipLaunchKernelGGL(quat_field_kernel<float>, dim3(grid_for(k)), dim3(kBlock), 0,
                           as_stream(stream), view_of<float>(h), ids, k,
                           static_cast<float *>(io), set);
    return launched(h, who);
}

// The options' fields: which option owns each, what the refusal says while
// that option is not enabled, and whether its words are i32 (two of them,
// moved by waypoint_field_kernel) or f32 (six, moved by wind_field_kernel).
struct OptionField {
    int field, kind;
    bool i32;
    const char *missing;
};
constexpr OptionField kOptionFields[] = {
    {DR_FIELD_WIND, dr_handle::OPT_WIND, false,
     ": wind exists only after a non-neutral dr_set_wind"},
    {DR_FIELD_WAYPOINT, dr_handle::OPT_WAYPOINT, true,
     ": waypoint exists only after dr_set_waypoints"},
    {DR_FIELD_AIRFRAME, dr_handle::OPT_AIRFRAME, false,
     ": airframe exists only after a non-neutral dr_set_airframe"}};

// DR_FIELD_WIND / _WAYPOINT / _AIRFRAME of dr_get_state / dr_gather_state /
// dr_set_state.
int option_field(dr_handle *h, const char *who, const OptionField &f, const int32_t *ids,
                 int64_t k, void *io, int set, void *stream) {
    if (h->opt_kind != f.kind) return fail(h, DR_ERR_UNSUPPORTED, std::string(who) + f.missing);
    if (k == 0) return DR_OK;
    DeviceGuard g(h->cfg.device);
    if (f.i32)
        hipLaunchKernelGGL(waypoint_field_kernel, dim3(grid_for(k)), dim3(kBlock), 0,
                           as_stream(stream), static_cast<int32_t *>(h->opt), h->stride, h->n,
                           ids, k, static_cast<int32_t *>(io), set);
    else
        hipLaunchKernelGGL(wind_field_kernel, dim3(grid_for(k)), dim3(kBlock), 0,
                           as_stream(stream), static_cast<float *>(h->opt), h->stride, h->n, ids,
                           k, static_cast<float *>(io), set);
    return launched(h, who);
}

// The fields kept beside the state arrays (motor, quat, the options'), for
// env j (ids null) or env ids[j] of k rows.  False if `field` is none of
// them; else true, with the call's result in *rc.
bool side_field(dr_handle *h, const char *who, int field, const int32_t *ids, int64_t k,
                void *io, int set, void *stream, int *rc) {
    if (field == DR_FIELD_MOTOR) {
        *rc = motor_field(h, who, ids, k, static_cast<float *>(io), set, stream);
        return true;
    }
    if (field == DR_FIELD_QUAT) {
        *rc = quat_field(h, who, ids, k, io, set, stream);
        return true;
    }
    for (const OptionField &f : kOptionFields) {
        if (field != f.field) continue;
        *rc = option_field(h, who, f, ids, k, io, set, stream);
        return true;
    }
    return false;
}

// The rk4 variant keeps a quaternion where the others keep Euler angles.
int euler_refused(dr_handle *h, const char *who, int field) {
    if (field == DR_FIELD_EULER && h->cfg.variant == DR_VARIANT_RK4)
        return fail(h, DR_ERR_UNSUPPORTED,
                    std::string(who) + ": DR_VARIANT_RK4 has no Euler angles; use DR_FIELD_QUAT");
    return DR_OK;
}

int check_rng(dr_handle *h) {
    if (h->cfg.rng_mode == DR_RNG_HOST_UNIFORMS && h->host_u == nullptr &&
        h->cfg.variant != DR_VARIANT_VECTORIZED)
        return fail(h, DR_ERR_INVALID,
                    "rng_mode DR_RNG_HOST_UNIFORMS: call dr_set_reset_uniforms first");
    return DR_OK;
}

// A handle has one of wind, a waypoint course and randomised airframes:
// `who` (which enables `mine`) is refused while another is enabled.
int option_conflict(dr_handle *h, const char *who, int mine) {
    static const char *const kHas[] = {nullptr, ": the handle has wind enabled",
                                       ": the handle is on a waypoint course",
                                       ": the handle has airframes enabled"};
    if (h->opt_kind == dr_handle::OPT_NONE || h->opt_kind == mine) return DR_OK;
    return fail(h, DR_ERR_UNSUPPORTED, std::string(who) + kHas[h->opt_kind]);
}

// Enable a filled option (wind, airframe): allocate its six f32 arrays, take
// the new parameters (`apply`), and give every env's current episode its
// words now, so that they are a function of (key, env, episode) whenever the
// option was switched on.  The state may be in use on any stream: drain, fill,
// drain.  On failure the handle is left without the option.
template <typename Apply>
int enable_option(dr_handle *h, int kind, const char *who, Apply &&apply) {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)6 * h->stride * sizeof(float));
    if (e != hipSuccess)
        return fail(h, DR_ERR_NOMEM, std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
    apply();
    e = hipDeviceSynchronize();
    h->opt = p;
    h->opt_kind = kind;
    int rc = e == hipSuccess ? launch_option_fill(h, nullptr, nullptr)
                             : fail(h, DR_ERR_HIP, hipGetErrorString(e));
    if (rc == DR_OK) {
        e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = fail(h, DR_ERR_HIP, hipGetErrorString(e));
    }
    if (rc != DR_OK) {
        h->opt = nullptr;
        h->opt_kind = dr_handle::OPT_NONE;
        (void)hipFree(p);
    }
    return rc;
}

}  // namespace

extern "C" {

int dr_abi_version(void) { return DR_ABI_VERSION; }

int dr_create(const dr_config *cfg_in, dr_handle **out) {
    if (!cfg_in || !out) return fail(nullptr, DR_ERR_INVALID, "dr_create: null argument");
    *out = nullptr;
    dr_config cfg = *cfg_in;
    if (cfg.num_envs < 1) return fail(nullptr, DR_ERR_INVALID, "dr_create: num_envs must be >= 1");
    if (cfg.variant != DR_VARIANT_GYM && cfg.variant != DR_VARIANT_VECTORIZED &&
        cfg.variant != DR_VARIANT_MOVING && cfg.variant != DR_VARIANT_SMOOTH &&
        cfg.variant != DR_VARIANT_TAG && cfg.variant != DR_VARIANT_RK4)
        return fail(nullptr, DR_ERR_INVALID, "dr_create: unknown variant");
    if (cfg.state_dtype != DR_STATE_F64 && cfg.state_dtype != DR_STATE_F32)
        return fail(nullptr, DR_ERR_INVALID, "dr_create: unknown state_dtype");
    if (cfg.rng_mode != DR_RNG_PHILOX && cfg.rng_mode != DR_RNG_HOST_UNIFORMS)
        return fail(nullptr, DR_ERR_INVALID, "dr_create: unknown rng_mode");
    // 32-bit per-array byte offsets in the step kernel (float4 actions:
    // 16 B x 2^28 = 4 GiB); shard larger batches over several handles
    if (cfg.num_envs > (int64_t)1 << 28)
        return fail(nullptr, DR_ERR_INVALID, "dr_create: num_envs above 2^28 per handle");
    // envs 2j and 2j+1 (global ids) are a pair, and a pair shares a wave
    if (cfg.variant == DR_VARIANT_TAG && ((cfg.num_envs & 1) || (cfg.env_id_offset & 1)))
        return fail(nullptr, DR_ERR_INVALID,
                    "dr_create: DR_VARIANT_TAG needs even num_envs and env_id_offset");
    if (cfg.max_steps == 0) cfg.max_steps = cfg.variant == DR_VARIANT_VECTORIZED ? 1000 : 200;
    if (cfg.max_steps < 0) return fail(nullptr, DR_ERR_INVALID, "dr_create: max_steps < 0");
    if (cfg.dt == 0.0) cfg.dt = kDt;
    if (cfg.variant == DR_VARIANT_VECTORIZED) cfg.auto_reset = 0;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, DR_ERR_HIP, "dr_create: no HIP device available");
    if (cfg.device < 0 || cfg.device >= ndev)
        return fail(nullptr, DR_ERR_INVALID, "dr_create: device ordinal out of range");

    dr_handle *h = new (std::nothrow) dr_handle();
    if (!h) return fail(nullptr, DR_ERR_NOMEM, "dr_create: host allocation failed");
    h->cfg = cfg;
    h->n = cfg.num_envs;
    // SoA arrays are `stride` elements apart.  A pure power-of-two spacing
    // puts the 17 concurrently streamed arrays at congruent addresses (same
    // HBM channel bits); a stride padded to skew them was an A/B build that
    // never became the default.
    h->stride = (cfg.num_envs + 63) / 64 * 64;
    h->obs_dim =
        for_variant(cfg.variant, [](auto var) { return Traits<decltype(var)::value>::OD; });
    // Launch form by batch size, from the measured sweep
    // (scripts/micro/ab_sweep.sh, profiles/r01_env_launch_sweep.txt):
    // [0, 384k) 64 rows/wave; [384k, 1.5M) 32 + nontemporal state loads;
    // [1.5M, 3M) 32; [3M, ...) 64 + nontemporal state loads.
    // The moving variant (9 more f32 arrays per env) and the f32 state mode
    // have sweeps of their own: moving always 64 rows/wave, nontemporal
    // state loads from 384k envs up; f32 state 64 rows/wave with plain loads
    // below 3M envs, 32 + nontemporal loads from 3M up.
    {
        const int64_t n = cfg.num_envs, k = (int64_t)1 << 10;
        if (cfg.variant == DR_VARIANT_MOVING) {
            h->rpw = 64;
            h->nt_loads = n >= 384 * k;
        } else if (cfg.state_dtype == DR_STATE_F32) {
            h->rpw = n >= 3072 * k ? 32 : 64;
            h->nt_loads = n >= 3072 * k;
        } else {
            h->rpw = (n >= 384 * k && n < 3072 * k) ? 32 : 64;
            h->nt_loads = (n >= 384 * k && n < 1536 * k) || n >= 3072 * k;
        }
    }
    if (const char *r = std::getenv("DRONERL_ROWS_PER_WAVE")) {
        const int v = std::atoi(r);
        if (v == 32 || v == 64) h->rpw = v;
    }
    if (const char *r = std::getenv("DRONERL_NT_LOADS")) h->nt_loads = std::atoi(r) != 0;

    DeviceGuard g(cfg.device);
    const size_t bytes = state_bytes(h->stride, cfg.state_dtype, cfg.variant);
    hipError_t e = hipMalloc(&h->mem, bytes);
    if (e != hipSuccess) {
        delete h;
        return fail(nullptr, DR_ERR_NOMEM, std::string("dr_create: hipMalloc: ") + hipGetErrorString(e));
    }
    // Constructor reset (drone.py:46): ep_num 0 -> 1.
    const int mode = cfg.rng_mode == DR_RNG_PHILOX ? 0 : 2;
    int rc = dispatch_reset(h, nullptr, nullptr, mode, 1, nullptr);
    if (rc == DR_OK) {
        e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = fail(h, DR_ERR_HIP, hipGetErrorString(e));
    }
    if (rc != DR_OK) {
        set_global_error(h->err);
        (void)hipFree(h->mem);
        delete h;
        return rc;
    }
    *out = h;
    return DR_OK;
}

int dr_destroy(dr_handle *h) {
    if (!h) return DR_OK;
    DeviceGuard g(h->cfg.device);
    if (h->mem) {
        // The caller's streams may still use the state: drain first.
        (void)hipDeviceSynchronize();
        (void)hipFree(h->mem);
        if (h->opt) (void)hipFree(h->opt);
    }
    delete h;
    return DR_OK;
}

int64_t dr_num_envs(const dr_handle *h) { return h ? h->n : -1; }
int dr_obs_dim(const dr_handle *h) { return h ? h->obs_dim : -1; }

int dr_reset(dr_handle *h, float *obs_out, void *stream) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_reset: null handle");
    if (!obs_out) return fail(h, DR_ERR_INVALID, "dr_reset: obs_out is null");
    int rc = check_rng(h);
    if (rc) return rc;
    DeviceGuard g(h->cfg.device);
    return dispatch_reset(h, nullptr, obs_out, h->host_u ? 1 : 0, 0, as_stream(stream));
}

int dr_reset_masked(dr_handle *h, const uint8_t *mask, float *obs_out, void *stream) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_reset_masked: null handle");
    if (!mask) return fail(h, DR_ERR_INVALID, "dr_reset_masked: mask is null");
    if (h->cfg.variant == DR_VARIANT_VECTORIZED)
        return fail(h, DR_ERR_UNSUPPORTED, "dr_reset_masked: vectorized variant resets globally");
    int rc = check_rng(h);
    if (rc) return rc;
    DeviceGuard g(h->cfg.device);
    return dispatch_reset(h, mask, obs_out, h->host_u ? 1 : 0, 0, as_stream(stream));
}

static int step_common(dr_handle *h, const float *actions, float *obs_out,
                       float *rew_out, uint8_t *done_out, float *term_obs_out,
                       float *ep_ret_out, int32_t *ep_len_out, bool mon,
                       void *stream, uint8_t *trunc_out = nullptr) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_step: null handle");
    if (!actions || !obs_out || !rew_out || !done_out)
        return fail(h, DR_ERR_INVALID, "dr_step: actions/obs/rew/done must be non-null");
    if (((uintptr_t)actions) & 15)
        return fail(h, DR_ERR_INVALID, "dr_step: actions must be 16-byte aligned");
    if (mon && (!ep_ret_out || !ep_len_out))
        return fail(h, DR_ERR_INVALID, "dr_step_monitored: episode outputs must be non-null");
    if (h->cfg.auto_reset) {
        int rc = check_rng(h);
        if (rc) return rc;
    }
    StepIO io{actions, obs_out, rew_out, done_out, term_obs_out, ep_ret_out,
              ep_len_out, h->cfg.auto_reset, trunc_out};
    DeviceGuard g(h->cfg.device);
    return mon ? dispatch_step<true>(h, io, as_stream(stream))
               : dispatch_step<false>(h, io, as_stream(stream));
}

int dr_step(dr_handle *h, const float *actions, float *obs_out, float *rew_out,
            uint8_t *done_out, float *terminal_obs_out, void *stream) {
    return step_common(h, actions, obs_out, rew_out, done_out, terminal_obs_out,
                       nullptr, nullptr, false, stream);
}

int dr_step_monitored(dr_handle *h, const float *actions, float *obs_out,
                      float *rew_out, uint8_t *done_out, float *terminal_obs_out,
                      float *ep_return_out, int32_t *ep_length_out, void *stream) {
    return step_common(h, actions, obs_out, rew_out, done_out, terminal_obs_out,
                       ep_return_out, ep_length_out, true, stream);
}

int dr_step_monitored_trunc(dr_handle *h, const float *actions, float *obs_out,
                            float *rew_out, uint8_t *done_out, float *terminal_obs_out,
                            float *ep_return_out, int32_t *ep_length_out,
                            uint8_t *truncated_out, void *stream) {
    if (!truncated_out)
        return fail(h, DR_ERR_INVALID, "dr_step_monitored_trunc: truncated_out is null");
    return step_common(h, actions, obs_out, rew_out, done_out, terminal_obs_out,
                       ep_return_out, ep_length_out, true, stream, truncated_out);
}

static int rollout_common(dr_handle *h, int32_t k, RolloutIO io, bool gen, void *stream,
                          void *start_event = nullptr, void *stop_event = nullptr) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_rollout: null handle");
    if (k < 0) return fail(h, DR_ERR_INVALID, "dr_rollout: k < 0");
    if (!io.obs || !io.rew || !io.done)
        return fail(h, DR_ERR_INVALID, "dr_rollout: obs/rew/done must be non-null");
    if (!gen && !io.actions) return fail(h, DR_ERR_INVALID, "dr_rollout: actions is null");
    if ((((uintptr_t)io.actions) & 15) || (((uintptr_t)io.act_out) & 15))
        return fail(h, DR_ERR_INVALID, "dr_rollout: actions must be 16-byte aligned");
    // per-step output offsets t * n are formed in 64 bits, the per-env
    // offset in 32 (as dr_step); K * n rows must still fit one allocation
    if ((int64_t)k * h->n > ((int64_t)1 << 31))
        return fail(h, DR_ERR_INVALID, "dr_rollout: k * num_envs above 2^31");
    if (h->cfg.variant != DR_VARIANT_VECTORIZED && h->cfg.auto_reset &&
        h->cfg.rng_mode != DR_RNG_PHILOX)
        return fail(h, DR_ERR_UNSUPPORTED,
                    "dr_rollout: host-supplied reset uniforms change per step; use dr_step");
    if (k == 0) return DR_OK;
    io.k = k;
    io.auto_reset = h->cfg.auto_reset;
    DeviceGuard g(h->cfg.device);
    const hipEvent_t e0 = static_cast<hipEvent_t>(start_event);
    const hipEvent_t e1 = static_cast<hipEvent_t>(stop_event);
    return gen ? dispatch_rollout<true>(h, io, as_stream(stream), e0, e1)
               : dispatch_rollout<false>(h, io, as_stream(stream), e0, e1);
}

int dr_rollout(dr_handle *h, int32_t k, const float *actions, float *obs_out, float *rew_out,
               uint8_t *done_out, void *stream) {
    RolloutIO io{};
    io.actions = actions;
    io.obs = obs_out;
    io.rew = rew_out;
    io.done = done_out;
    return rollout_common(h, k, io, false, stream);
}

int dr_rollout_timed(dr_handle *h, int32_t k, const float *actions, float *obs_out,
                     float *rew_out, uint8_t *done_out, void *stream, void *start_event,
                     void *stop_event) {
    RolloutIO io{};
    io.actions = actions;
    io.obs = obs_out;
    io.rew = rew_out;
    io.done = done_out;
    return rollout_common(h, k, io, false, stream, start_event, stop_event);
}

int dr_rollout_random(dr_handle *h, int32_t k, uint64_t action_seed, int64_t action_step0,
                      float lo, float hi, float *actions_out, float *obs_out, float *rew_out,
                      uint8_t *done_out, void *stream) {
    RolloutIO io{};
    io.act_out = actions_out;
    io.obs = obs_out;
    io.rew = rew_out;
    io.done = done_out;
    io.a_k0 = (uint32_t)action_seed;
    io.a_k1 = (uint32_t)(action_seed >> 32);
    io.a_step0 = (uint64_t)action_step0;
    io.a_lo = lo;
    io.a_span = hi - lo;
    return rollout_common(h, k, io, true, stream);
}

int dr_get_state(dr_handle *h, int field, void *out, void *stream) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_get_state: null handle");
    if (!out) return fail(h, DR_ERR_INVALID, "dr_get_state: out is null");
    int src;
    if (side_field(h, "dr_get_state", field, nullptr, h->n, out, 0, stream, &src)) return src;
    if (int rc = euler_refused(h, "dr_get_state", field)) return rc;
    if (field < DR_FIELD_POS || field > DR_FIELD_MOTION)
        return fail(h, DR_ERR_INVALID, "dr_get_state: unknown field");
    if (field == DR_FIELD_MOTION && h->cfg.variant != DR_VARIANT_MOVING)
        return fail(h, DR_ERR_INVALID, "dr_get_state: motion exists only for DR_VARIANT_MOVING");
    DeviceGuard g(h->cfg.device);
    if (h->cfg.state_dtype == DR_STATE_F64)
        hipLaunchKernelGGL(get_field_kernel<double>, dim3(grid_for(h->n)), dim3(kBlock), 0,
                           as_stream(stream), view_of<double>(h), field, out);
    else
        hipLaunchKernelGGL(get_field_kernel<float>, dim3(grid_for(h->n)), dim3(kBlock), 0,
                           as_stream(stream), view_of<float>(h), field, out);
    return launched(h, "get_field");
}

int dr_gather_state(dr_handle *h, int field, const int32_t *env_ids, int64_t k, void *out,
                    void *stream) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_gather_state: null handle");
    if (!env_ids || !out || k < 0) return fail(h, DR_ERR_INVALID, "dr_gather_state: bad arguments");
    int src;
    if (side_field(h, "dr_gather_state", field, env_ids, k, out, 0, stream, &src)) return src;
    if (int rc = euler_refused(h, "dr_gather_state", field)) return rc;
    if (field < DR_FIELD_POS || field > DR_FIELD_MOTION)
        return fail(h, DR_ERR_INVALID, "dr_gather_state: unknown field");
    if (field == DR_FIELD_MOTION && h->cfg.variant != DR_VARIANT_MOVING)
        return fail(h, DR_ERR_INVALID, "dr_gather_state: motion exists only for DR_VARIANT_MOVING");
    if (k == 0) return DR_OK;
    DeviceGuard g(h->cfg.device);
    if (h->cfg.state_dtype == DR_STATE_F64)
        hipLaunchKernelGGL(gather_field_kernel<double>, dim3(grid_for(k)), dim3(kBlock), 0,
                           as_stream(stream), view_of<double>(h), field, env_ids, k, out);
    else
        hipLaunchKernelGGL(gather_field_kernel<float>, dim3(grid_for(k)), dim3(kBlock), 0,
                           as_stream(stream), view_of<float>(h), field, env_ids, k, out);
    return launched(h, "gather_field");
}

int dr_set_state(dr_handle *h, int field, const void *in, void *stream) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_set_state: null handle");
    if (!in) return fail(h, DR_ERR_INVALID, "dr_set_state: in is null");
    int src;
    if (side_field(h, "dr_set_state", field, nullptr, h->n, const_cast<void *>(in), 1, stream, &src))
        return src;
    if (int rc = euler_refused(h, "dr_set_state", field)) return rc;
    if (field < DR_FIELD_POS || field > DR_FIELD_MOTION)
        return fail(h, DR_ERR_INVALID, "dr_set_state: unknown field");
    if (field == DR_FIELD_MOTION && h->cfg.variant != DR_VARIANT_MOVING)
        return fail(h, DR_ERR_INVALID, "dr_set_state: motion exists only for DR_VARIANT_MOVING");
    DeviceGuard g(h->cfg.device);
    if (h->cfg.state_dtype == DR_STATE_F64)
        hipLaunchKernelGGL(set_field_kernel<double>, dim3(grid_for(h->n)), dim3(kBlock), 0,
                           as_stream(stream), view_of<double>(h), field, in);
    else
        hipLaunchKernelGGL(set_field_kernel<float>, dim3(grid_for(h->n)), dim3(kBlock), 0,
                           as_stream(stream), view_of<float>(h), field, in);
    return launched(h, "set_field");
}

int dr_set_reset_uniforms(dr_handle *h, const double *u_dev) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_set_reset_uniforms: null handle");
    if (h->cfg.rng_mode != DR_RNG_HOST_UNIFORMS)
        return fail(h, DR_ERR_INVALID, "dr_set_reset_uniforms: handle uses DR_RNG_PHILOX");
    h->host_u = u_dev;
    return DR_OK;
}

int dr_set_seed(dr_handle *h, uint64_t seed) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_set_seed: null handle");
    h->cfg.seed = seed;
    return DR_OK;
}

int dr_set_smoothing(dr_handle *h, float alpha, float rate_penalty) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_set_smoothing: null handle");
    // written so that NaN fails every test
    if (!(alpha > 0.0f && alpha <= 1.0f))
        return fail(h, DR_ERR_INVALID, "dr_set_smoothing: alpha must be in (0, 1]");
    if (!(rate_penalty >= 0.0f && rate_penalty <= 3.4028234663852886e38f))
        return fail(h, DR_ERR_INVALID, "dr_set_smoothing: rate_penalty must be finite and >= 0");
    if (h->cfg.variant != DR_VARIANT_SMOOTH)
        return fail(h, DR_ERR_UNSUPPORTED, "dr_set_smoothing: only DR_VARIANT_SMOOTH has a motor lag");
    h->alpha = alpha;
    h->rate_penalty = rate_penalty;
    return DR_OK;
}

int dr_get_smoothing(const dr_handle *h, float *alpha, float *rate_penalty) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_get_smoothing: null handle");
    if (h->cfg.variant != DR_VARIANT_SMOOTH) return DR_ERR_UNSUPPORTED;
    if (alpha) *alpha = h->alpha;
    if (rate_penalty) *rate_penalty = h->rate_penalty;
    return DR_OK;
}

int dr_set_tag(dr_handle *h, float tag_radius, float crash_penalty) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_set_tag: null handle");
    // written so that NaN fails every test
    if (!(tag_radius > 0.0f && tag_radius <= 3.4028234663852886e38f))
        return fail(h, DR_ERR_INVALID, "dr_set_tag: tag_radius must be finite and > 0");
    if (!(crash_penalty >= 0.0f && crash_penalty <= 3.4028234663852886e38f))
        return fail(h, DR_ERR_INVALID, "dr_set_tag: crash_penalty must be finite and >= 0");
    if (h->cfg.variant != DR_VARIANT_TAG)
        return fail(h, DR_ERR_UNSUPPORTED, "dr_set_tag: only DR_VARIANT_TAG has pairs");
    h->tag_radius = tag_radius;
    h->crash_penalty = crash_penalty;
    return DR_OK;
}

int dr_get_tag(const dr_handle *h, float *tag_radius, float *crash_penalty) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_get_tag: null handle");
    if (h->cfg.variant != DR_VARIANT_TAG) return DR_ERR_UNSUPPORTED;
    if (tag_radius) *tag_radius = h->tag_radius;
    if (crash_penalty) *crash_penalty = h->crash_penalty;
    return DR_OK;
}

int dr_set_wind(dr_handle *h, float drag, float wind_speed, float gust_sigma, float gust_rate) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_set_wind: null handle");
    // written so that NaN fails every test
    constexpr float kMax = 3.4028234663852886e38f;
    if (!(drag >= 0.0f && drag <= kMax))
        return fail(h, DR_ERR_INVALID, "dr_set_wind: drag must be finite and >= 0");
    if (!(wind_speed >= 0.0f && wind_speed <= kMax))
        return fail(h, DR_ERR_INVALID, "dr_set_wind: wind_speed must be finite and >= 0");
    if (!(gust_sigma >= 0.0f && gust_sigma <= kMax))
        return fail(h, DR_ERR_INVALID, "dr_set_wind: gust_sigma must be finite and >= 0");
    if (!(gust_rate >= 0.0f && gust_rate <= 1.0f))
        return fail(h, DR_ERR_INVALID, "dr_set_wind: gust_rate must be in [0, 1]");
    // the explicit drag update must not overshoot the air's velocity
    if (!((double)drag * h->cfg.dt <= 1.0))
        return fail(h, DR_ERR_INVALID, "dr_set_wind: drag * dt must be <= 1");
    if (h->cfg.variant != DR_VARIANT_GYM)
        return fail(h, DR_ERR_UNSUPPORTED, "dr_set_wind: only DR_VARIANT_GYM has wind");
    // the gust counter carries the step counter in its low 24 bits
    if (h->cfg.max_steps >= (1 << 24))
        return fail(h, DR_ERR_UNSUPPORTED, "dr_set_wind: max_steps must be below 2^24");
    const bool neutral =
        drag == 0.0f && wind_speed == 0.0f && gust_sigma == 0.0f && gust_rate == 0.0f;
    if (!neutral)
        if (int rc = option_conflict(h, "dr_set_wind", dr_handle::OPT_WIND)) return rc;
    auto apply = [&] {
        h->drag = drag;
        h->wind_speed = wind_speed;
        h->gust_sigma = gust_sigma;
        h->gust_rate = gust_rate;
        h->gust_b = 1.0f - gust_rate;
        h->gust_c = (float)((double)gust_sigma *
                            std::sqrt(3.0 * (1.0 - (double)h->gust_b * (double)h->gust_b)));
    };
    DeviceGuard g(h->cfg.device);
    if (h->opt_kind != dr_handle::OPT_WIND && !neutral)
        return enable_option(h, dr_handle::OPT_WIND, "dr_set_wind", apply);
    apply();
    return DR_OK;
}

int dr_get_wind(const dr_handle *h, float *drag, float *wind_speed, float *gust_sigma,
                float *gust_rate) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_get_wind: null handle");
    if (h->cfg.variant != DR_VARIANT_GYM) return DR_ERR_UNSUPPORTED;
    if (drag) *drag = h->drag;
    if (wind_speed) *wind_speed = h->wind_speed;
    if (gust_sigma) *gust_sigma = h->gust_sigma;
    if (gust_rate) *gust_rate = h->gust_rate;
    return DR_OK;
}

int dr_set_waypoints(dr_handle *h, float reach_radius, float reach_bonus) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_set_waypoints: null handle");
    // written so that NaN fails every test
    constexpr float kMax = 3.4028234663852886e38f;
    if (!(reach_radius > 0.0f && reach_radius <= kMax))
        return fail(h, DR_ERR_INVALID, "dr_set_waypoints: reach_radius must be finite and > 0");
    if (!(reach_bonus >= 0.0f && reach_bonus <= kMax))
        return fail(h, DR_ERR_INVALID, "dr_set_waypoints: reach_bonus must be finite and >= 0");
    if (h->cfg.variant != DR_VARIANT_GYM)
        return fail(h, DR_ERR_UNSUPPORTED,
                    "dr_set_waypoints: only DR_VARIANT_GYM has waypoint courses");
    if (int rc = option_conflict(h, "dr_set_waypoints", dr_handle::OPT_WAYPOINT)) return rc;
    // the waypoint counter carries the index, below the step limit, in its
    // low 24 bits
    if (h->cfg.max_steps >= (1 << 24))
        return fail(h, DR_ERR_UNSUPPORTED, "dr_set_waypoints: max_steps must be below 2^24");
    if (h->opt_kind != dr_handle::OPT_WAYPOINT) {
        // j = q = 0 for every env; the state may be in use on any stream:
        // drain, allocate and clear, drain
        DeviceGuard g(h->cfg.device);
        int32_t *w = nullptr;
        const size_t bytes = (size_t)2 * h->stride * sizeof(int32_t);
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return fail(h, DR_ERR_HIP, hipGetErrorString(e));
        e = hipMalloc(reinterpret_cast<void **>(&w), bytes);
        if (e != hipSuccess)
            return fail(h, DR_ERR_NOMEM,
                        std::string("dr_set_waypoints: hipMalloc: ") + hipGetErrorString(e));
        e = hipMemset(w, 0, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void)hipFree(w);
            return fail(h, DR_ERR_HIP, hipGetErrorString(e));
        }
        h->opt = w;
        h->opt_kind = dr_handle::OPT_WAYPOINT;
    }
    h->reach_radius = reach_radius;
    h->reach_bonus = reach_bonus;
    return DR_OK;
}

int dr_get_waypoints(const dr_handle *h, float *reach_radius, float *reach_bonus) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_get_waypoints: null handle");
    if (h->cfg.variant != DR_VARIANT_GYM) return DR_ERR_UNSUPPORTED;
    if (reach_radius) *reach_radius = h->reach_radius;
    if (reach_bonus) *reach_bonus = h->reach_bonus;
    return DR_OK;
}

int dr_set_airframe(dr_handle *h, float mass_spread, float inertia_spread, float motor_spread) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_set_airframe: null handle");
    // written so that NaN fails every test
    if (!(mass_spread >= 0.0f && mass_spread <= 0.9f))
        return fail(h, DR_ERR_INVALID, "dr_set_airframe: mass_spread must be in [0, 0.9]");
    if (!(inertia_spread >= 0.0f && inertia_spread <= 0.9f))
        return fail(h, DR_ERR_INVALID, "dr_set_airframe: inertia_spread must be in [0, 0.9]");
    if (!(motor_spread >= 0.0f && motor_spread <= 0.9f))
        return fail(h, DR_ERR_INVALID, "dr_set_airframe: motor_spread must be in [0, 0.9]");
    if (h->cfg.variant != DR_VARIANT_GYM)
        return fail(h, DR_ERR_UNSUPPORTED,
                    "dr_set_airframe: only DR_VARIANT_GYM has airframe randomisation");
    if (int rc = option_conflict(h, "dr_set_airframe", dr_handle::OPT_AIRFRAME)) return rc;
    const bool neutral = mass_spread == 0.0f && inertia_spread == 0.0f && motor_spread == 0.0f;
    const float old[3] = {h->mass_spread, h->inertia_spread, h->motor_spread};
    auto apply = [&] {
        h->mass_spread = mass_spread;
        h->inertia_spread = inertia_spread;
        h->motor_spread = motor_spread;
    };
    DeviceGuard g(h->cfg.device);
    if (h->opt_kind != dr_handle::OPT_AIRFRAME && !neutral) {
        const int rc = enable_option(h, dr_handle::OPT_AIRFRAME, "dr_set_airframe", apply);
        if (rc != DR_OK) {
            h->mass_spread = old[0];
            h->inertia_spread = old[1];
            h->motor_spread = old[2];
        }
        return rc;
    }
    apply();
    return DR_OK;
}

int dr_get_airframe(const dr_handle *h, float *mass_spread, float *inertia_spread,
                    float *motor_spread) {
    if (!h) return fail(nullptr, DR_ERR_INVALID, "dr_get_airframe: null handle");
    if (h->cfg.variant != DR_VARIANT_GYM) return DR_ERR_UNSUPPORTED;
    if (mass_spread) *mass_spread = h->mass_spread;
    if (inertia_spread) *inertia_spread = h->inertia_spread;
    if (motor_spread) *motor_spread = h->motor_spread;
    return DR_OK;
}

int dr_random_actions(int64_t n, uint64_t seed, int64_t env_id_offset,
                      int64_t step, float lo, float hi, float *out, void *stream) {
    if (n < 0 || !out) return fail(nullptr, DR_ERR_INVALID, "dr_random_actions: bad arguments");
    if (((uintptr_t)out) & 15) return fail(nullptr, DR_ERR_INVALID, "dr_random_actions: out must be 16-byte aligned");
    if (n == 0) return DR_OK;
    hipLaunchKernelGGL(random_actions_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
                       as_stream(stream), n, (uint32_t)seed, (uint32_t)(seed >> 32),
                       env_id_offset, (uint64_t)step, lo, hi - lo,
                       reinterpret_cast<float4 *>(out));
    return launched(nullptr, "random_actions");
}

#if DR_STAMPS
int dr_diag_stamps(void *host_out, size_t bytes) {
    hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), bytes, 0,
                                       hipMemcpyDeviceToHost);
    return e == hipSuccess ? DR_OK : DR_ERR_HIP;
}
#endif

const char *dr_last_error(const dr_handle *h) {
    return h ? h->err.c_str() : global_error();
}

}  // extern "C"

// MPPIPlanner (dr_mppi_*): its own file, this translation unit (the model it
// plans on is physics_step above).
#include "planner.hip"

// GradPlanner (dr_gplan_*): the adjoint of physics_step and the planner on it,
// after planner.hip, whose clip it shares.
#include "grad_planner.hip"
