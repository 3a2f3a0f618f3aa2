// VecNormalize for MI355X (gfx950): running observation / reward
// normalisation with its statistics as device state.
//
// Restates stable-baselines3's VecNormalize + RunningMeanStd (not vendored in
// the reference; the contract is the text of DESIGN.md section 21, pinned by
// the NumPy restatement tests/vecnorm_ref.py).  All statistics are f64.
//
// One step is at most three launches, none of which waits for the host:
//   1. vecnorm_partial_kernel   one block per 256 rows: the tile is read once,
//      flat and coalesced, into LDS; (n, mean, M2) of every obs column of the
//      tile (two passes over the LDS tile), and of the tile's updated returns,
//      go to the workspace
//   2. vecnorm_finish_kernel    one block, one wave per column: the partials
//      merge in a fixed order (chan_merge) and obs_rms / ret_rms advance
//   3. vecnorm_apply_kernel     the normalise pass over obs, rewards and the
//      done rows of the terminal obs; returns[done] <- 0
// With frozen statistics (or both norms off) only the third runs.  Nothing is
// kept between launches but obs_rms, ret_rms and returns; there is no atomic:
// every result is a function of the inputs alone, so reruns and graph replays
// are bitwise equal.
//
// Built as part of ppo_kernels.hip's translation unit (included at its end):
// every build of the library that lists the three sources, the sanitizer build
// of the host code among them, then exports these entry points too.  Every
// name at namespace scope here carries a vn / Vn prefix.
//
// Non-finite inputs get no special treatment: a NaN or inf in a column
// poisons that column's mean and variance for good, as in SB3 (the clip
// passes NaN through, like np.clip).

#include <cmath>
#include <string>

#include "common.h"

#pragma clang fp contract(off)

namespace dr {
namespace {

constexpr int kVnRows = 256;      // rows per block of the partial / apply kernels
constexpr int kVnMaxDim = 24;     // widest obs row
constexpr int kVnFinish = 1024;   // threads of the finish kernel: 16 waves

int vn_fail(const std::string &msg) {
    set_global_error(msg);
    return DR_ERR_INVALID;
}

int vn_check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_global_error(std::string(what) + ": " + hipGetErrorString(e));
        return DR_ERR_HIP;
    }
    return DR_OK;
}

inline hipStream_t vn_stream(void *s) { return static_cast<hipStream_t>(s); }

// chan_merge that takes b as it is when a is empty (so a lone partial passes
// through every level bit for bit).
__device__ inline void vn_merge(double &n, double &mu, double &M2, double nb_, double mb,
                                double m2b) {
    if (n == 0.0) {
        n = nb_;
        mu = mb;
        M2 = m2b;
        return;
    }
    chan_merge(n, mu, M2, nb_, mb, m2b);
}

// RunningMeanStd.update_from_moments on (count, mean, var) with a batch of
// bc rows whose moments are (bm, M2): bv = M2 / bc.
__device__ inline void vn_rms_update(double count, double &mean, double &var, double bc, double bm,
                                  double M2) {
    const double bv = M2 / bc;
    const double d = bm - mean;
    const double tot = count + bc;
    const double new_mean = mean + d * bc / tot;
    const double new_var = (var * count + bv * bc + d * d * count * bc / tot) / tot;
    mean = new_mean;
    var = new_var;
}

// ---------------------------------------------------------------------------
// 1. partials.  Block b owns rows [256 b, 256 b + rows).  Its rows * D floats
// are contiguous: thread t loads floats t, t + 256, ... (coalesced dwords)
// into an LDS tile.  Column c is then split over S = 256 / D slices: thread
// s * D + c walks rows s, s + S, ... of the tile (consecutive threads read
// consecutive words: no bank conflict).  Two passes over the tile: the slice
// sums, added in slice order by thread c, give the tile's column mean; the
// slices' squared deviations from THAT mean, added in slice order, are the
// tile's M2 (deviations from one common mean simply add: no merge, and one
// division per column).
// The returns column: returns <- returns * gamma + reward per row, then the
// same two passes over a fixed 256-leaf sum tree.
// part holds (D + 1) triples (n, mean, M2) per block: columns 0..D-1, then
// the returns.
// ---------------------------------------------------------------------------
__device__ inline double vn_tree_sum(double *sa, int t) {
    __syncthreads();
    for (int h = kVnRows / 2; h > 0; h >>= 1) {
        if (t < h) sa[t] += sa[t + h];
        __syncthreads();
    }
    const double r = sa[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kVnRows) void vecnorm_partial_kernel(
    int64_t n, int D, const float *obs, const float *rew, double *returns, double gamma,
    int do_obs, int do_ret, double *part) {
    __shared__ float tile[kVnRows * kVnMaxDim];
    __shared__ double sa[kVnRows], smean[kVnMaxDim];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kVnRows;
    const int rows = (int)((n - row0) < (int64_t)kVnRows ? (n - row0) : (int64_t)kVnRows);
    double *out = part + (int64_t)blockIdx.x * (D + 1) * 3;
    if (do_obs) {
        const float *src = obs + row0 * D;
        const int nf = rows * D;
        for (int j = t; j < nf; j += kVnRows) tile[j] = src[j];
        __syncthreads();
        const int S = kVnRows / D;
        const bool active = t < S * D;
        const int c = t % D, s = t / D;
        double acc = 0.0;
        if (active)
            for (int r = s; r < rows; r += S) acc += (double)tile[r * D + c];
        sa[t] = acc;
        __syncthreads();
        if (t < D) {
            double tot = sa[t];
            for (int q = 1; q < S; ++q) tot += sa[q * D + t];
            smean[t] = tot / (double)rows;
        }
        __syncthreads();
        acc = 0.0;
        if (active) {
            const double mu = smean[c];
            for (int r = s; r < rows; r += S) {
                const double dx = (double)tile[r * D + c] - mu;
                acc += dx * dx;
            }
        }
        sa[t] = acc;
        __syncthreads();
        if (t < D) {
            double M2 = sa[t];
            for (int q = 1; q < S; ++q) M2 += sa[q * D + t];
            out[3 * t + 0] = (double)rows;
            out[3 * t + 1] = smean[t];
            out[3 * t + 2] = M2;
        }
        __syncthreads();
    }
    if (do_ret) {
        double x = 0.0;
        if (t < rows) {
            x = returns[row0 + t] * gamma + (double)rew[row0 + t];
            returns[row0 + t] = x;
        }
        sa[t] = x;
        const double mu = vn_tree_sum(sa, t) / (double)rows;
        const double dx = x - mu;
        sa[t] = t < rows ? dx * dx : 0.0;
        const double M2 = vn_tree_sum(sa, t);
        if (t == 0) {
            out[3 * D + 0] = (double)rows;
            out[3 * D + 1] = mu;
            out[3 * D + 2] = M2;
        }
    }
}

// ---------------------------------------------------------------------------
// 2. finish.  One block of 16 waves; wave w takes columns w, w + 16 (column D
// is the returns).  Lane l merges partials l, l + 64, ... in that order, then
// the 64 lanes merge through a fixed shuffle tree; lane 0 advances the
// statistic.  obs_rms' count is read by everyone before the barrier and
// written by thread 0 after it.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kVnFinish) void vecnorm_finish_kernel(
    int64_t n, int D, int64_t nb, const double *part, int do_obs, int do_ret, double *obs_rms,
    double *ret_rms) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double count = obs_rms[0];
    __syncthreads();
    for (int c = wave; c <= D; c += kVnFinish / 64) {
        if (c < D ? !do_obs : !do_ret) continue;
        double a = 0.0, am = 0.0, a2 = 0.0;
        for (int64_t b = lane; b < nb; b += 64) {
            const double *p = part + (b * (D + 1) + c) * 3;
            vn_merge(a, am, a2, p[0], p[1], p[2]);
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double bn = __shfl_down(a, off, 64);
            const double bm = __shfl_down(am, off, 64);
            const double b2 = __shfl_down(a2, off, 64);
            vn_merge(a, am, a2, bn, bm, b2);
        }
        if (lane == 0) {
            if (c < D) {
                double mean = obs_rms[1 + c], var = obs_rms[1 + D + c];
                vn_rms_update(count, mean, var, (double)n, am, a2);
                obs_rms[1 + c] = mean;
                obs_rms[1 + D + c] = var;
            } else {
                const double rc = ret_rms[0];
                double mean = ret_rms[1], var = ret_rms[2];
                vn_rms_update(rc, mean, var, (double)n, am, a2);
                ret_rms[0] = rc + (double)n;
                ret_rms[1] = mean;
                ret_rms[2] = var;
            }
        }
    }
    if (do_obs && threadIdx.x == 0) obs_rms[0] = count + (double)n;
}

// ---------------------------------------------------------------------------
// 3. normalise.  The partial kernel's geometry: block b streams its rows * D
// floats flat (coalesced dwords), the column's mean and sqrt(var + eps) from
// LDS.  out = f32(clip((f64(x) - mean) / sd, -clip, clip)), one IEEE f64
// division per element, NaN passed through.
// ---------------------------------------------------------------------------
__device__ inline float vn_norm(float x, double mean, double sd, double clip) {
    double y = ((double)x - mean) / sd;
    y = y < -clip ? -clip : (y > clip ? clip : y);
    return (float)y;
}

struct VnApplyArgs {
    int64_t n;
    int D;
    const float *obs;        // may alias obs_out
    const float *rew;        // nullable; may alias rew_out
    const uint8_t *dones;    // with rew
    const float *term;       // nullable
    int norm_obs, norm_rew;
    int zero_returns;        // 1: returns <- 0 for every env (the reset form)
    double clip_obs, clip_rew, eps;
    const double *obs_rms, *ret_rms;
    double *returns;         // nullable (dr_vecnorm_apply)
    float *obs_out, *rew_out, *term_out;
};

__global__ __launch_bounds__(kVnRows) void vecnorm_apply_kernel(VnApplyArgs a) {
    __shared__ double smean[kVnMaxDim], ssd[kVnMaxDim];
    const int t = threadIdx.x, D = a.D;
    const int64_t row0 = (int64_t)blockIdx.x * kVnRows;
    const int rows = (int)((a.n - row0) < (int64_t)kVnRows ? (a.n - row0) : (int64_t)kVnRows);
    if (a.norm_obs && t < D) {
        smean[t] = a.obs_rms[1 + t];
        ssd[t] = sqrt(a.obs_rms[1 + D + t] + a.eps);
    }
    __syncthreads();
    const int nf = rows * D;
    const int64_t e0 = row0 * D;
    if (a.norm_obs) {
        // element j = t + 256 i of the tile is column (t + 256 i) mod D
        const int hop = kVnRows % D;
        int c = t % D;
        for (int j = t; j < nf; j += kVnRows) {
            a.obs_out[e0 + j] = vn_norm(a.obs[e0 + j], smean[c], ssd[c], a.clip_obs);
            c += hop;
            if (c >= D) c -= D;
        }
    } else if (a.obs_out != a.obs) {
        for (int j = t; j < nf; j += kVnRows) a.obs_out[e0 + j] = a.obs[e0 + j];
    }
    if (a.term) {
        for (int j = t; j < nf; j += kVnRows) {
            const int r = j / D, c = j - r * D;
            if (a.dones[row0 + r]) {
                const float x = a.term[e0 + j];
                a.term_out[e0 + j] = a.norm_obs ? vn_norm(x, smean[c], ssd[c], a.clip_obs) : x;
            }
        }
    }
    if (t < rows) {
        const int64_t i = row0 + t;
        if (a.rew) {
            const float r = a.rew[i];
            if (a.norm_rew) {
                const double sd = sqrt(a.ret_rms[2] + a.eps);
                a.rew_out[i] = vn_norm(r, 0.0, sd, a.clip_rew);
            } else if (a.rew_out != a.rew) {
                a.rew_out[i] = r;
            }
            if (a.dones[i]) a.returns[i] = 0.0;
        } else if (a.zero_returns) {
            a.returns[i] = 0.0;
        }
    }
}

// out = f32(f64(x) * sqrt(var + eps) + mean): VecNormalize.unnormalize_obs.
__global__ __launch_bounds__(kVnRows) void vecnorm_unapply_kernel(int64_t n, int D,
                                                                   const float *x,
                                                                   const double *obs_rms,
                                                                   double eps, float *out) {
    __shared__ double smean[kVnMaxDim], ssd[kVnMaxDim];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kVnRows;
    const int rows = (int)((n - row0) < (int64_t)kVnRows ? (n - row0) : (int64_t)kVnRows);
    if (t < D) {
        smean[t] = obs_rms[1 + t];
        ssd[t] = sqrt(obs_rms[1 + D + t] + eps);
    }
    __syncthreads();
    const int nf = rows * D;
    const int64_t e0 = row0 * D;
    for (int j = t; j < nf; j += kVnRows) {
        const int c = j % D;
        out[e0 + j] = (float)((double)x[e0 + j] * ssd[c] + smean[c]);
    }
}

__global__ __launch_bounds__(kVnRows) void vecnorm_init_kernel(int64_t n, int D, double *obs_rms,
                                                                double *ret_rms,
                                                                double *returns) {
    const int64_t i = (int64_t)blockIdx.x * kVnRows + threadIdx.x;
    if (i < n) returns[i] = 0.0;
    if (blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t == 0) {
            obs_rms[0] = 1e-4;
            ret_rms[0] = 1e-4;
            ret_rms[1] = 0.0;
            ret_rms[2] = 1.0;
        }
        if (t < D) {
            obs_rms[1 + t] = 0.0;
            obs_rms[1 + D + t] = 1.0;
        }
    }
}

inline int64_t vn_blocks(int64_t n) { return (n + kVnRows - 1) / kVnRows; }

inline bool vn_pos_finite(double x) { return x > 0.0 && std::isfinite(x); }

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_vecnorm_workspace_bytes(int64_t n, int64_t obs_dim) {
    if (n < 1 || obs_dim < 1 || obs_dim > kVnMaxDim) return 0;
    return sizeof(double) * 3 * (size_t)(obs_dim + 1) * (size_t)vn_blocks(n);
}

int dr_vecnorm_init(int64_t n, int64_t obs_dim, double *obs_rms, double *ret_rms,
                    double *returns, void *stream) {
    if (n < 1) return vn_fail("dr_vecnorm_init: n must be >= 1");
    if (obs_dim < 1 || obs_dim > kVnMaxDim)
        return vn_fail("dr_vecnorm_init: obs_dim must be in [1, 24]");
    if (vn_blocks(n) > 0x7fffffff) return vn_fail("dr_vecnorm_init: n too large");
    if (!obs_rms || !ret_rms || !returns)
        return vn_fail("dr_vecnorm_init: obs_rms, ret_rms and returns must be non-null");
    hipLaunchKernelGGL(vecnorm_init_kernel, dim3((unsigned)vn_blocks(n)), dim3(kVnRows), 0,
                       vn_stream(stream), n, (int)obs_dim, obs_rms, ret_rms, returns);
    return vn_check_launch("dr_vecnorm_init");
}

int dr_vecnorm_step(int64_t n, int64_t obs_dim, const float *obs, const float *rewards,
                    const uint8_t *dones, const float *terminal_obs, int flags, double gamma,
                    double clip_obs, double clip_reward, double epsilon, double *obs_rms,
                    double *ret_rms, double *returns, float *obs_out, float *rew_out,
                    float *terminal_obs_out, void *workspace, size_t workspace_bytes,
                    void *stream) {
    if (n < 1) return vn_fail("dr_vecnorm_step: n must be >= 1");
    if (obs_dim < 1 || obs_dim > kVnMaxDim)
        return vn_fail("dr_vecnorm_step: obs_dim must be in [1, 24]");
    if (vn_blocks(n) > 0x7fffffff) return vn_fail("dr_vecnorm_step: n too large");
    if (flags & ~(DR_VECNORM_OBS | DR_VECNORM_REWARD | DR_VECNORM_TRAINING))
        return vn_fail("dr_vecnorm_step: unknown flag bits");
    if (!obs || !obs_out) return vn_fail("dr_vecnorm_step: obs and obs_out must be non-null");
    if (!obs_rms || !ret_rms || !returns)
        return vn_fail("dr_vecnorm_step: obs_rms, ret_rms and returns must be non-null");
    if (rewards && (!dones || !rew_out))
        return vn_fail("dr_vecnorm_step: rewards need dones and rew_out");
    if (!rewards && (terminal_obs || terminal_obs_out))
        return vn_fail("dr_vecnorm_step: the reset form (rewards == NULL) takes no terminal obs");
    if ((terminal_obs != nullptr) != (terminal_obs_out != nullptr))
        return vn_fail("dr_vecnorm_step: terminal_obs and terminal_obs_out go together");
    if (!std::isfinite(gamma)) return vn_fail("dr_vecnorm_step: gamma must be finite");
    if (!vn_pos_finite(clip_obs)) return vn_fail("dr_vecnorm_step: clip_obs must be > 0 and finite");
    if (!vn_pos_finite(clip_reward))
        return vn_fail("dr_vecnorm_step: clip_reward must be > 0 and finite");
    if (!(epsilon >= 0.0) || !std::isfinite(epsilon))
        return vn_fail("dr_vecnorm_step: epsilon must be >= 0 and finite");
    const size_t need = dr_vecnorm_workspace_bytes(n, obs_dim);
    if (!workspace || workspace_bytes < need || (((uintptr_t)workspace) & 7))
        return vn_fail("dr_vecnorm_step: workspace too small (dr_vecnorm_workspace_bytes) or "
                       "not 8-byte aligned");
    const int D = (int)obs_dim;
    const bool training = flags & DR_VECNORM_TRAINING;
    const int norm_obs = (flags & DR_VECNORM_OBS) ? 1 : 0;
    const int norm_rew = (flags & DR_VECNORM_REWARD) ? 1 : 0;
    const int do_obs = training && norm_obs;
    const int do_ret = training && norm_rew && rewards;
    hipStream_t st = vn_stream(stream);
    const int64_t nb = vn_blocks(n);
    if (do_obs || do_ret) {
        double *part = static_cast<double *>(workspace);
        hipLaunchKernelGGL(vecnorm_partial_kernel, dim3((unsigned)nb), dim3(kVnRows), 0, st, n, D,
                           obs, rewards, returns, gamma, do_obs, do_ret, part);
        if (int rc = vn_check_launch("dr_vecnorm_step (partials)")) return rc;
        hipLaunchKernelGGL(vecnorm_finish_kernel, dim3(1), dim3(kVnFinish), 0, st, n, D, nb,
                           (const double *)part, do_obs, do_ret, obs_rms, ret_rms);
        if (int rc = vn_check_launch("dr_vecnorm_step (finish)")) return rc;
    }
    VnApplyArgs a;
    a.n = n;
    a.D = D;
    a.obs = obs;
    a.rew = rewards;
    a.dones = dones;
    a.term = terminal_obs;
    a.norm_obs = norm_obs;
    a.norm_rew = norm_rew;
    a.zero_returns = rewards ? 0 : 1;
    a.clip_obs = clip_obs;
    a.clip_rew = clip_reward;
    a.eps = epsilon;
    a.obs_rms = obs_rms;
    a.ret_rms = ret_rms;
    a.returns = returns;
    a.obs_out = obs_out;
    a.rew_out = rew_out;
    a.term_out = terminal_obs_out;
    hipLaunchKernelGGL(vecnorm_apply_kernel, dim3((unsigned)nb), dim3(kVnRows), 0, st, a);
    return vn_check_launch("dr_vecnorm_step (normalise)");
}

int dr_vecnorm_apply(int64_t m, int64_t obs_dim, const float *obs, const double *obs_rms,
                     double clip_obs, double epsilon, float *obs_out, void *stream) {
    if (m < 1) return vn_fail("dr_vecnorm_apply: m must be >= 1");
    if (obs_dim < 1 || obs_dim > kVnMaxDim)
        return vn_fail("dr_vecnorm_apply: obs_dim must be in [1, 24]");
    if (vn_blocks(m) > 0x7fffffff) return vn_fail("dr_vecnorm_apply: m too large");
    if (!obs || !obs_rms || !obs_out)
        return vn_fail("dr_vecnorm_apply: obs, obs_rms and obs_out must be non-null");
    if (!vn_pos_finite(clip_obs))
        return vn_fail("dr_vecnorm_apply: clip_obs must be > 0 and finite");
    if (!(epsilon >= 0.0) || !std::isfinite(epsilon))
        return vn_fail("dr_vecnorm_apply: epsilon must be >= 0 and finite");
    VnApplyArgs a = {};
    a.n = m;
    a.D = (int)obs_dim;
    a.obs = obs;
    a.norm_obs = 1;
    a.clip_obs = clip_obs;
    a.clip_rew = 1.0;
    a.eps = epsilon;
    a.obs_rms = obs_rms;
    a.obs_out = obs_out;
    hipLaunchKernelGGL(vecnorm_apply_kernel, dim3((unsigned)vn_blocks(m)), dim3(kVnRows), 0,
                       vn_stream(stream), a);
    return vn_check_launch("dr_vecnorm_apply");
}

int dr_vecnorm_unapply(int64_t m, int64_t obs_dim, const float *obs_norm, const double *obs_rms,
                       double epsilon, float *obs_out, void *stream) {
    if (m < 1) return vn_fail("dr_vecnorm_unapply: m must be >= 1");
    if (obs_dim < 1 || obs_dim > kVnMaxDim)
        return vn_fail("dr_vecnorm_unapply: obs_dim must be in [1, 24]");
    if (vn_blocks(m) > 0x7fffffff) return vn_fail("dr_vecnorm_unapply: m too large");
    if (!obs_norm || !obs_rms || !obs_out)
        return vn_fail("dr_vecnorm_unapply: obs_norm, obs_rms and obs_out must be non-null");
    if (!(epsilon >= 0.0) || !std::isfinite(epsilon))
        return vn_fail("dr_vecnorm_unapply: epsilon must be >= 0 and finite");
    hipLaunchKernelGGL(vecnorm_unapply_kernel, dim3((unsigned)vn_blocks(m)), dim3(kVnRows), 0,
                       vn_stream(stream), m, (int)obs_dim, obs_norm, obs_rms, epsilon, obs_out);
    return vn_check_launch("dr_vecnorm_unapply");
}

}  // extern "C"
