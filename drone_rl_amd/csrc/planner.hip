// MPPIPlanner for MI355X (gfx950): sampled trajectory planning on the env's
// own physics (the law is restated in NumPy by
// tests/mppi_ref.py, and its model, noise and cost must match dr_step bit for
// bit).
//
// One block of S threads per env, one sample per lane.  The env's nominal
// action sequence U (H x 4 f32) and its observation sit in LDS and are read
// by broadcast; the 15 state words of a sample live in registers for the whole
// horizon, stepped by physics_step<double, DR_VARIANT_GYM>, the function the
// env kernels call.  Between the loads at the top and the stores at the bottom
// the kernel touches no global memory.
//   pass 1  every lane flies its sample H steps and accumulates its return J;
//           a crashed sample keeps stepping with the accumulation masked, so
//           the horizon loop is uniform;
//   weights Jmax, then w = exp((J - Jmax) / lambda) and W = sum w: per-wave
//           DPP butterflies, then across the waves through LDS in wave order;
//   pass 2  every lane draws its actions again (the same Philox blocks: an
//           action costs one block, keeping H x 4 of them would cost 4 H
//           registers) and the 4 H weighted sums are reduced the same way.
// No atomics and a fixed order everywhere: reruns and graph replays are
// bitwise equal.
//
// Built as part of env_kernels.hip's translation unit, the one place where the
// model function is visible.  Every name at namespace scope here carries a
// pl / Pl prefix.

#include <cmath>
#include <string>

#include "common.h"

#pragma clang fp contract(off)

namespace dr {
namespace {

constexpr int kPlMaxH = DR_MPPI_MAX_HORIZON;
constexpr int kPlMaxThreads = DR_MPPI_MAX_SAMPLES;
constexpr int kPlMaxWaves = kPlMaxThreads / 64;
constexpr float kPlMotorMax = (float)(3 * kMass * kG / 4.0);   // action_space.high

int pl_fail(const std::string &msg) {
    set_global_error(msg);
    return DR_ERR_INVALID;
}

struct PlArgs {
    int H;
    float sig;                 // sigma' = f32(sigma sqrt 3)
    double lambda, crash_cost, terminal_weight;
    uint32_t k0, k1;
    uint64_t gid0;
    const float *obs;
    const uint8_t *dones;      // nullable
    float *nominal;            // (n, H, 4)
    uint32_t *calls;           // (n,)
    float *actions;            // (n, 4)
    double *costs;             // (n, S), nullable
    double disc[kPlMaxH];      // gamma^h
};

// np.clip's result for every x, NaN and -0 included
__device__ inline float pl_clip(float x) {
    return x < 0.0f ? 0.0f : (x > kPlMotorMax ? kPlMotorMax : x);
}

// Sample s's action at step h: the nominal itself for s = 0, else the nominal
// plus sigma' pm1(w_k) of the block (calls, gid, TAG_PLAN | (s H + h)); clipped.
__device__ inline float4 pl_action(const PlArgs &a, float4 u, uint32_t calls, uint64_t gid, int s,
                                   int idx) {
    const u32x4 w = philox4x32_10(
        u32x4{calls, (uint32_t)gid, (uint32_t)(gid >> 32), TAG_PLAN | (uint32_t)idx}, a.k0, a.k1);
    const float e0 = a.sig * wind_pm1(w.x), e1 = a.sig * wind_pm1(w.y);
    const float e2 = a.sig * wind_pm1(w.z), e3 = a.sig * wind_pm1(w.w);
    const bool nom = s == 0;
    return float4{pl_clip(nom ? u.x : u.x + e0), pl_clip(nom ? u.y : u.y + e1),
                  pl_clip(nom ? u.z : u.z + e2), pl_clip(nom ? u.w : u.w + e3)};
}

template <int CTRL>
__device__ inline double pl_dpp(double x) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
__device__ inline double pl_xor16(double x) {
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(x), 0x401F);
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(x), 0x401F);
    return __hiloint2double(hi, lo);
}
__device__ inline double pl_lane(double x, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane),
                            __builtin_amdgcn_readlane(__double2loint(x), lane));
}

// Sum / maximum over the 64 lanes, wave-uniform.  Fixed butterfly order:
// quad xor 1, quad xor 2, half-row mirror, row mirror (DPP), xor 16, then
// lane 0 with lane 32.
__device__ inline double pl_wave_sum(double x) {
    x = x + pl_dpp<0xB1>(x);
    x = x + pl_dpp<0x4E>(x);
    x = x + pl_dpp<0x141>(x);
    x = x + pl_dpp<0x140>(x);
    x = x + pl_xor16(x);
    return pl_lane(x, 0) + pl_lane(x, 32);
}
__device__ inline double pl_wave_max(double x) {
    x = fmax(x, pl_dpp<0xB1>(x));
    x = fmax(x, pl_dpp<0x4E>(x));
    x = fmax(x, pl_dpp<0x141>(x));
    x = fmax(x, pl_dpp<0x140>(x));
    x = fmax(x, pl_xor16(x));
    return fmax(pl_lane(x, 0), pl_lane(x, 32));
}

__global__ __launch_bounds__(kPlMaxThreads) void mppi_step_kernel(PlArgs a) {
    __shared__ float4 U[kPlMaxH];
    __shared__ float ob[16];
    __shared__ double red[2][kPlMaxWaves];
    __shared__ double part[kPlMaxH * 4][kPlMaxWaves];
    const int t = threadIdx.x, S = blockDim.x, H = a.H;
    const int wave = t >> 6, nw = S >> 6;
    const bool lane0 = (t & 63) == 0;
    const int64_t env = blockIdx.x;
    float *const nom = a.nominal + env * (H * 4);
    float *const Uf = reinterpret_cast<float *>(U);

    // every load: the nominal (hover where the obs opens a new episode), the
    // observation, the call count
    const bool fresh = a.dones && a.dones[env];
    for (int j = t; j < H * 4; j += S) Uf[j] = fresh ? kHover32 : nom[j];
    if (t < 15) ob[t] = a.obs[env * 15 + t];
    const uint32_t calls = a.calls[env];
    const uint64_t gid = a.gid0 + (uint64_t)env;
    __syncthreads();

    // the start state the policy's observation describes
    double st[F_N];
#pragma unroll
    for (int k = 0; k < 12; ++k) st[k] = (double)ob[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) st[F_TGT + k] = (double)ob[k] + (double)ob[12 + k];

    // pass 1: the sample's return
    double J = 0.0;
    bool alive = true;
    for (int h = 0; h < H; ++h) {
        const float4 act = pl_action(a, U[h], calls, gid, t, t * H + h);
        bool crash;
        const double r = physics_step<double, DR_VARIANT_GYM>(st, act, (double)kDt, crash);
        const double term = a.disc[h] * ((double)(float)r - (crash ? a.crash_cost : 0.0));
        J = alive ? J + term : J;
        alive = alive && !crash;
    }
    {
        const double dx = st[F_POS + 0] - st[F_TGT + 0];
        const double dy = st[F_POS + 1] - st[F_TGT + 1];
        const double dz = st[F_POS + 2] - st[F_TGT + 2];
        const double d = m_sqrt((dx * dx + dy * dy) + dz * dz);
        J = alive ? J - a.terminal_weight * d : J;
    }

    // the weights
    const bool ok = J == J;
    const double wm = pl_wave_max(ok ? J : -INFINITY);
    if (lane0) red[0][wave] = wm;
    __syncthreads();
    double Jmax = red[0][0];
    for (int w = 1; w < nw; ++w) Jmax = fmax(Jmax, red[0][w]);
    // no sample with a finite return: the nominal stays, nothing is averaged
    const bool valid = Jmax - Jmax == 0.0;
    if (valid) {
        const double wt = ok ? exp((J - Jmax) / a.lambda) : 0.0;
        const double ws = pl_wave_sum(wt);
        if (lane0) red[1][wave] = ws;
        // pass 2: the weighted sums of the redrawn actions
        for (int h = 0; h < H; ++h) {
            const float4 act = pl_action(a, U[h], calls, gid, t, t * H + h);
            const double s0 = pl_wave_sum(wt * (double)act.x);
            const double s1 = pl_wave_sum(wt * (double)act.y);
            const double s2 = pl_wave_sum(wt * (double)act.z);
            const double s3 = pl_wave_sum(wt * (double)act.w);
            if (lane0) {
                part[4 * h + 0][wave] = s0;
                part[4 * h + 1][wave] = s1;
                part[4 * h + 2][wave] = s2;
                part[4 * h + 3][wave] = s3;
            }
        }
    }
    __syncthreads();

    // the stores: this call's action, the shifted nominal, the call count
    if (a.costs) a.costs[env * S + t] = J;
    if (t == 0) a.calls[env] = calls + 1u;
    if (valid) {
        double W = red[1][0];
        for (int w = 1; w < nw; ++w) W = W + red[1][w];
        for (int j = t; j < H * 4; j += S) {
            double acc = part[j][0];
            for (int w = 1; w < nw; ++w) acc = acc + part[j][w];
            const float u = (float)(acc / W);
            const int h = j >> 2, k = j & 3;
            if (h == 0) a.actions[env * 4 + k] = u;
            else nom[j - 4] = u;
            if (h == H - 1) nom[j] = u;
        }
    } else {
        for (int j = t; j < H * 4; j += S) {
            nom[j] = Uf[j];
            if (j < 4) a.actions[env * 4 + j] = pl_clip(Uf[j]);
        }
    }
}

__global__ __launch_bounds__(kBlock) void mppi_reset_kernel(int64_t n, int64_t words,
                                                            float *nominal, uint32_t *calls) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < words) nominal[i] = kHover32;
    if (i < n) calls[i] = 0u;
}

inline bool pl_nonneg_finite(double x) { return x >= 0.0 && std::isfinite(x); }

// The checks both entry points share.
int pl_check(const char *who, const dr_mppi_config *cfg, int64_t n, const float *nominal,
             const uint32_t *calls) {
    const std::string w(who);
    if (!cfg) return pl_fail(w + ": config must be non-null");
    if (n < 1 || n > 0x7fffffff) return pl_fail(w + ": n must be in [1, 2^31)");
    const int S = cfg->samples;
    if (S != 64 && S != 128 && S != 256 && S != 512 && S != 1024)
        return pl_fail(w + ": samples must be one of 64, 128, 256, 512, 1024");
    if (cfg->horizon < 1 || cfg->horizon > kPlMaxH)
        return pl_fail(w + ": horizon must be in [1, 32]");
    if (!pl_nonneg_finite(cfg->sigma)) return pl_fail(w + ": sigma must be >= 0 and finite");
    if (!(cfg->temperature > 0.0) || !std::isfinite(cfg->temperature))
        return pl_fail(w + ": temperature must be > 0 and finite");
    if (!(cfg->gamma > 0.0 && cfg->gamma <= 1.0)) return pl_fail(w + ": gamma must be in (0, 1]");
    if (!pl_nonneg_finite(cfg->crash_cost))
        return pl_fail(w + ": crash_cost must be >= 0 and finite");
    if (!pl_nonneg_finite(cfg->terminal_weight))
        return pl_fail(w + ": terminal_weight must be >= 0 and finite");
    if (!nominal) return pl_fail(w + ": nominal must be non-null");
    if (!calls) return pl_fail(w + ": calls must be non-null");
    return DR_OK;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

int dr_mppi_reset(const dr_mppi_config *cfg, int64_t n, float *nominal, uint32_t *calls,
                  void *stream) {
    if (int rc = pl_check("dr_mppi_reset", cfg, n, nominal, calls)) return rc;
    const int64_t words = n * cfg->horizon * 4;
    hipLaunchKernelGGL(mppi_reset_kernel, dim3(grid_for(words)), dim3(kBlock), 0,
                       as_stream(stream), n, words, nominal, calls);
    return launched(nullptr, "dr_mppi_reset");
}

int dr_mppi_step(const dr_mppi_config *cfg, int64_t n, const float *obs, const uint8_t *dones,
                 float *nominal, uint32_t *calls, float *actions_out, double *costs_out,
                 void *stream) {
    if (int rc = pl_check("dr_mppi_step", cfg, n, nominal, calls)) return rc;
    if (!obs) return pl_fail("dr_mppi_step: obs must be non-null");
    if (!actions_out) return pl_fail("dr_mppi_step: actions_out must be non-null");
    PlArgs a{};
    a.H = cfg->horizon;
    // sigma' = sigma sqrt(3) in f64, rounded once: u in [-1, 1) has std 1 / sqrt(3)
    a.sig = (float)(cfg->sigma * std::sqrt(3.0));
    a.lambda = cfg->temperature;
    a.crash_cost = cfg->crash_cost;
    a.terminal_weight = cfg->terminal_weight;
    a.k0 = (uint32_t)cfg->seed;
    a.k1 = (uint32_t)(cfg->seed >> 32);
    a.gid0 = (uint64_t)cfg->env_id_offset;
    a.obs = obs;
    a.dones = dones;
    a.nominal = nominal;
    a.calls = calls;
    a.actions = actions_out;
    a.costs = costs_out;
    // disc[h] = gamma^h as the running product: one f64 rounding per step
    double d = 1.0;
    for (int h = 0; h < a.H; ++h) {
        a.disc[h] = d;
        d = d * cfg->gamma;
    }
    hipLaunchKernelGGL(mppi_step_kernel, dim3((unsigned)n), dim3(cfg->samples), 0,
                       as_stream(stream), a);
    return launched(nullptr, "dr_mppi_step");
}

}  // extern "C"
