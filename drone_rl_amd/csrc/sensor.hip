// SensorModel for MI355X (gfx950): observation noise, bias and latency between
// the env and the policy, with its state on the device (DESIGN.md section 23;
// the law is restated in NumPy by tests/sensor_ref.py and must match it bit
// for bit).
//
// Per env the wrapper owns (ep, s, d), a per-column bias and a ring of
// L = delay_hi + 1 clean observation rows; it reads none of the env's
// counters.  One launch per dr_sensor_step and one per dr_sensor_reset, the
// same kernel: a block of 256 threads owns 64 consecutive envs.
//   * rows move flat: thread t touches floats t, t + 256, ... of the tile's
//     64 * D contiguous floats (coalesced dwords) of obs, bias, out, and of
//     ring plane k at (k * n + row) * D + c -- envs of one launch sit at
//     different s, so each row's slot differs, but a row is contiguous;
//   * the Philox blocks are one task per (row, quad of columns): 64 * D/4
//     tasks over the 256 threads, their errors e_c left in an LDS tile so
//     that a mirror column reads its source's e whatever quad it is in.
// Done rows are rare: the terminal delivery and the refill of all L slots run
// only for them (the terminal pass not at all in a tile without one).
// No atomics; every env is independent: reruns and graph replays are bitwise
// equal.
//
// Built as part of ppo_kernels.hip's translation unit, as vecnorm.hip is.
// Every name at namespace scope here carries an sn / Sn prefix.

#include <cmath>
#include <string>

#include "common.h"

#pragma clang fp contract(off)

namespace dr {
namespace {

constexpr int kSnRows = 64;       // envs per block
constexpr int kSnThreads = 256;
constexpr int kSnMaxDim = DR_SENSOR_MAX_DIM;
constexpr uint32_t kSnTag = 0x53000000u;     // TAG_SENSOR: delay (block 0), biases (1 + q)
constexpr uint32_t kSnNoiseTop = 0x60u;      // noise blocks: top byte 0x60 + q

int sn_fail(const std::string &msg) {
    set_global_error(msg);
    return DR_ERR_INVALID;
}

// f32(2u - 1) of a Philox word's 32-bit uniform (the wind option's pm1).
__device__ inline float sn_pm1(uint32_t w) { return (float)(2.0 * u01_w32(w) - 1.0); }

struct SnArgs {
    int64_t n;
    int D, L, Q;
    int reset;                 // 1: every env starts episode 0
    int lo, span;              // delay_lo, delay_hi - delay_lo + 1
    uint32_t k0, k1;
    uint64_t gid0;
    uint32_t live;             // bit q: quad q has a column with sigma or beta > 0
    const float *obs;
    const uint8_t *dones;
    const float *term;         // nullable
    int32_t *state;            // (3, n): ep, s, d
    float *bias;               // (n, D)
    float *ring;               // (L, n, D)
    float *out, *term_out;
    float sig[kSnMaxDim];      // sigma' = f32(sigma sqrt 3)
    float beta[kSnMaxDim];
    int32_t mirror[kSnMaxDim];
    uint32_t pass;             // bit c: the column is delivered unchanged
};

struct SnTile {
    float x[kSnRows * kSnMaxDim];      // the clean rows to deliver
    float e[kSnRows * kSnMaxDim];      // bias, then bias + noise
    float sig[kSnMaxDim], beta[kSnMaxDim];
    int mirror[kSnMaxDim];
    uint32_t ep[kSnRows];
    int s[kSnRows], d[kSnRows];
    int wr[kSnRows], rd[kSnRows];      // the ring slots the row writes / reads, once per row
    uint8_t start[kSnRows];            // the env starts an episode in this launch
};

inline __device__ int sn_mod(int a, int L) {
    int m = a % L;
    return m < 0 ? m + L : m;
}

// e[r][c] += sigma'_c * pm1(word c % 4 of the noise block (0x60 + c / 4, s))
// for the rows of the tile (only started ones with only_start).  `bump` is
// added to the row's count: the terminal delivery is the old episode's s + 1.
__device__ inline void sn_noise(const SnArgs &a, SnTile &T, int rows, int64_t row0, int bump,
                                bool only_start) {
    const int D = a.D, Q = a.Q;
    for (int task = threadIdx.x; task < rows * Q; task += kSnThreads) {
        const int r = task / Q, q = task - r * Q;
        if (!((a.live >> q) & 1u)) continue;
        if (only_start && !T.start[r]) continue;
        const uint64_t gid = a.gid0 + (uint64_t)(row0 + r);
        const uint32_t cnt = (uint32_t)(T.s[r] + bump) & 0xffffffu;
        const u32x4 w = philox4x32_10(
            u32x4{T.ep[r], (uint32_t)gid, (uint32_t)(gid >> 32),
                  ((kSnNoiseTop + (uint32_t)q) << 24) | cnt}, a.k0, a.k1);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = 4 * q + k;
            if (c < D) T.e[r * D + c] = T.e[r * D + c] + T.sig[c] * sn_pm1(ws[k]);
        }
    }
}

// out = x + e_c, or x - e_m for a mirror of column m; x itself for a column
// whose sigma and beta (its source's, for a mirror) are both zero.
__device__ inline float sn_deliver(const SnArgs &a, const SnTile &T, int j, int r, int c) {
    const float x = T.x[j];
    if ((a.pass >> c) & 1u) return x;
    const int m = T.mirror[c];
    return m < 0 ? x + T.e[j] : x - T.e[r * a.D + m];
}

// The flat walk of a tile: element j = t + 256 i is row j / D, column j % D.
#define SN_FLAT_BEGIN(nf, D)                                                     \
    {                                                                            \
        const int hop_c__ = kSnThreads % (D), hop_r__ = kSnThreads / (D);        \
        int r = threadIdx.x / (D), c = threadIdx.x - r * (D);                    \
        for (int j = threadIdx.x; j < (nf); j += kSnThreads) {
#define SN_FLAT_END(D)                                                           \
            c += hop_c__;                                                        \
            r += hop_r__;                                                        \
            if (c >= (D)) {                                                      \
                c -= (D);                                                        \
                r += 1;                                                          \
            }                                                                    \
        }                                                                        \
    }

__global__ __launch_bounds__(kSnThreads) void sensor_kernel(SnArgs a) {
    __shared__ SnTile T;
    const int t = threadIdx.x, D = a.D, L = a.L;
    const int64_t n = a.n;
    const int64_t row0 = (int64_t)blockIdx.x * kSnRows;
    const int rows = (int)((n - row0) < (int64_t)kSnRows ? (n - row0) : (int64_t)kSnRows);
    const int nf = rows * D;
    const int64_t e0 = row0 * D;
    const int64_t plane = n * D;
    if (t < D) {
        T.sig[t] = a.sig[t];
        T.beta[t] = a.beta[t];
        T.mirror[t] = a.mirror[t];
    }
    int started = 0;
    if (t < rows) {
        if (a.reset) {
            T.ep[t] = 0u;
            T.s[t] = 0;
            T.d[t] = 0;
            started = 1;
        } else {
            T.ep[t] = (uint32_t)a.state[row0 + t];
            T.s[t] = a.state[n + row0 + t];
            T.d[t] = a.state[2 * n + row0 + t];
            started = a.dones[row0 + t] ? 1 : 0;
        }
        T.start[t] = (uint8_t)started;
        // the terminal delivery's slot: the old episode at s + 1
        T.rd[t] = sn_mod(T.s[t] + 1 - T.d[t], L);
    }
    const int any_start = __syncthreads_or(started);

    // the delivery the old episode of a done env would have made at s + 1
    // with the terminal observation as that step's clean row
    if (a.term && any_start) {
        SN_FLAT_BEGIN(nf, D)
        if (T.start[r]) {
            const int d = T.d[r];
            T.e[j] = a.bias[e0 + j];
            T.x[j] = d == 0 ? a.term[e0 + j] : a.ring[(int64_t)T.rd[r] * plane + e0 + j];
        }
        SN_FLAT_END(D)
        __syncthreads();
        sn_noise(a, T, rows, row0, 1, true);
        __syncthreads();
        SN_FLAT_BEGIN(nf, D)
        if (T.start[r]) a.term_out[e0 + j] = sn_deliver(a, T, j, r, c);
        SN_FLAT_END(D)
        __syncthreads();
    }

    // the counters: an episode start draws its delay, everyone else counts on
    if (t < rows) {
        if (started) {
            const uint32_t ep = a.reset ? 0u : T.ep[t] + 1u;
            const uint64_t gid = a.gid0 + (uint64_t)(row0 + t);
            const u32x4 w = philox4x32_10(
                u32x4{ep, (uint32_t)gid, (uint32_t)(gid >> 32), kSnTag}, a.k0, a.k1);
            T.ep[t] = ep;
            T.s[t] = 0;
            T.d[t] = a.lo + (int)(((uint64_t)w.x * (uint64_t)a.span) >> 32);
            a.state[row0 + t] = (int32_t)ep;
            a.state[2 * n + row0 + t] = T.d[t];
        } else {
            T.s[t] += 1;
        }
        a.state[n + row0 + t] = T.s[t];
        T.wr[t] = sn_mod(T.s[t], L);
        T.rd[t] = sn_mod(T.s[t] - T.d[t], L);
    }
    __syncthreads();

    // an episode start's biases: block 1 + q, one task per (row, quad)
    if (any_start) {
        for (int task = t; task < rows * a.Q; task += kSnThreads) {
            const int r = task / a.Q, q = task - r * a.Q;
            if (!T.start[r]) continue;
            const uint64_t gid = a.gid0 + (uint64_t)(row0 + r);
            const u32x4 w = philox4x32_10(
                u32x4{T.ep[r], (uint32_t)gid, (uint32_t)(gid >> 32), kSnTag | (uint32_t)(1 + q)},
                a.k0, a.k1);
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 4 * q + k;
                if (c < D) T.e[r * D + c] = T.beta[c] * sn_pm1(ws[k]);
            }
        }
        __syncthreads();
    }

    // the clean row into the ring (every slot at an episode start), the row
    // of d steps ago out of it
    SN_FLAT_BEGIN(nf, D)
    {
        const float x = a.obs[e0 + j];
        float xr = x;
        if (T.start[r]) {
            a.bias[e0 + j] = T.e[j];
            for (int k = 0; k < L; ++k) a.ring[(int64_t)k * plane + e0 + j] = x;
        } else {
            const int wr = T.wr[r], rd = T.rd[r];
            T.e[j] = a.bias[e0 + j];
            a.ring[(int64_t)wr * plane + e0 + j] = x;
            if (rd != wr) xr = a.ring[(int64_t)rd * plane + e0 + j];
        }
        T.x[j] = xr;
    }
    SN_FLAT_END(D)
    __syncthreads();
    sn_noise(a, T, rows, row0, 0, false);
    __syncthreads();
    SN_FLAT_BEGIN(nf, D)
    a.out[e0 + j] = sn_deliver(a, T, j, r, c);
    SN_FLAT_END(D)
}

#undef SN_FLAT_BEGIN
#undef SN_FLAT_END

inline bool sn_nonneg_finite(float x) { return x >= 0.0f && std::isfinite(x); }

// The checks both entry points share, and the by-value kernel arguments.
int sn_prepare(const char *who, const dr_sensor_config *cfg, int64_t n, int64_t obs_dim,
               const float *obs, int32_t *state, float *bias, float *ring, float *obs_out,
               SnArgs &a) {
    const std::string w(who);
    if (!cfg) return sn_fail(w + ": config must be non-null");
    if (n < 1) return sn_fail(w + ": n must be >= 1");
    if (obs_dim < 1 || obs_dim > kSnMaxDim) return sn_fail(w + ": obs_dim must be in [1, 24]");
    if ((n + kSnRows - 1) / kSnRows > 0x7fffffff) return sn_fail(w + ": n too large");
    if (cfg->delay_lo < 0 || cfg->delay_hi < cfg->delay_lo || cfg->delay_hi > DR_SENSOR_MAX_DELAY)
        return sn_fail(w + ": delay needs 0 <= delay_lo <= delay_hi <= 15");
    const int D = (int)obs_dim;
    for (int c = 0; c < D; ++c) {
        if (!sn_nonneg_finite(cfg->sigma[c]))
            return sn_fail(w + ": sigma[" + std::to_string(c) + "] must be >= 0 and finite");
        if (!sn_nonneg_finite(cfg->beta[c]))
            return sn_fail(w + ": beta[" + std::to_string(c) + "] must be >= 0 and finite");
        if (cfg->mirror[c] < -1 || cfg->mirror[c] >= c)
            return sn_fail(w + ": mirror[" + std::to_string(c) + "] must be -1 or in [0, " +
                           std::to_string(c) + ")");
    }
    if (!obs || !obs_out) return sn_fail(w + ": obs and obs_out must be non-null");
    if (!state || !bias || !ring) return sn_fail(w + ": state, bias and ring must be non-null");
    a = SnArgs{};
    a.n = n;
    a.D = D;
    a.L = cfg->delay_hi + 1;
    a.Q = (D + 3) / 4;
    a.lo = cfg->delay_lo;
    a.span = cfg->delay_hi - cfg->delay_lo + 1;
    a.k0 = (uint32_t)cfg->seed;
    a.k1 = (uint32_t)(cfg->seed >> 32);
    a.gid0 = (uint64_t)cfg->env_id_offset;
    a.obs = obs;
    a.state = state;
    a.bias = bias;
    a.ring = ring;
    a.out = obs_out;
    for (int c = 0; c < D; ++c) {
        // sigma' = sigma sqrt(3) in f64, rounded once: u in [-1, 1) has std 1 / sqrt(3)
        a.sig[c] = (float)((double)cfg->sigma[c] * std::sqrt(3.0));
        a.beta[c] = cfg->beta[c];
        a.mirror[c] = cfg->mirror[c];
        if (cfg->sigma[c] != 0.0f || cfg->beta[c] != 0.0f) a.live |= 1u << (c / 4);
    }
    for (int c = 0; c < D; ++c) {
        const int m = cfg->mirror[c] < 0 ? c : cfg->mirror[c];
        if (cfg->sigma[m] == 0.0f && cfg->beta[m] == 0.0f) a.pass |= 1u << c;
    }
    return DR_OK;
}

int sn_launch(const char *who, const SnArgs &a, void *stream) {
    const unsigned blocks = (unsigned)((a.n + kSnRows - 1) / kSnRows);
    hipLaunchKernelGGL(sensor_kernel, dim3(blocks), dim3(kSnThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_global_error(std::string(who) + ": " + hipGetErrorString(e));
        return DR_ERR_HIP;
    }
    return DR_OK;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

int dr_sensor_reset(const dr_sensor_config *cfg, int64_t n, int64_t obs_dim, const float *obs,
                    int32_t *state, float *bias, float *ring, float *obs_out, void *stream) {
    SnArgs a;
    if (int rc = sn_prepare("dr_sensor_reset", cfg, n, obs_dim, obs, state, bias, ring, obs_out, a))
        return rc;
    a.reset = 1;
    return sn_launch("dr_sensor_reset", a, stream);
}

int dr_sensor_step(const dr_sensor_config *cfg, int64_t n, int64_t obs_dim, const float *obs,
                   const uint8_t *dones, const float *terminal_obs, int32_t *state, float *bias,
                   float *ring, float *obs_out, float *terminal_out, void *stream) {
    SnArgs a;
    if (int rc = sn_prepare("dr_sensor_step", cfg, n, obs_dim, obs, state, bias, ring, obs_out, a))
        return rc;
    if (!dones) return sn_fail("dr_sensor_step: dones must be non-null");
    if ((terminal_obs != nullptr) != (terminal_out != nullptr))
        return sn_fail("dr_sensor_step: terminal_obs and terminal_out go together");
    a.dones = dones;
    a.term = terminal_obs;
    a.term_out = terminal_out;
    return sn_launch("dr_sensor_step", a, stream);
}

}  // extern "C"
