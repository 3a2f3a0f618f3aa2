// KL control of the PPO optimizer step for MI355X (gfx950): SB3's target_kl
// early stop and a KL-adaptive learning rate, decided on the device by the
// launch that applies Adam (pinned by the NumPy
// restatement tests/kl_ref.py).
//
// The trainer owns a control block of S + 1 slots for an iteration of S
// optimizer steps, each slot (stopped u32, taken u32, lr f32, pad).  The
// Adam-apply launch of step j reads slot j and this step's approx_kl (final
// one launch earlier) and writes slot j + 1.  No launch reads a word another
// block of the same launch writes and there is no atomic: every block takes
// the same decision from the same words, so reruns and graph replays are
// bitwise equal.
//
// clip_adam_kl_kernel restates clip_adam_kernel's arithmetic word for word
// (this translation unit is compiled with contraction off, so an applied step
// is bitwise the ungated kernel's at the same step scalars); the ungated
// kernel and its entry points are left as they were.
//
// Built as part of ppo_kernels.hip's translation unit (included at its end),
// like vecnorm.hip.

#pragma clang fp contract(off)

namespace dr {
namespace {

struct KlGateArgs {
    const uint32_t *slot_in;     // slot j
    uint32_t *slot_out;          // slot j + 1
    const float *kl;             // this step's approx_kl
    const float *sched;          // (nsched, 2) dr_adam_schedule rows
    int nsched;
    int has_target, adaptive;
    float stop_kl, kl_high, kl_low, lr_min, lr_max;
};

__global__ __launch_bounds__(kBlock) void clip_adam_kl_kernel(
    int64_t n, float *__restrict__ p, float *__restrict__ g,
    float *__restrict__ m, float *__restrict__ v, const float *__restrict__ part,
    int nb, float max_norm, float w1, float beta2, float one_m_b2, float eps,
    float *norm_out, float gscale, KlGateArgs a) {
    // the decision: a function of slot j, kl and launch arguments alone,
    // formed by every thread alike
    const uint32_t stopped_in = a.slot_in[0];
    const uint32_t taken = a.slot_in[1];
    float lr = __uint_as_float(a.slot_in[2]);
    const float kl = *a.kl;
    // trip: false for NaN (a NaN kl does not stop, as in SB3)
    const bool trip = a.has_target && kl > a.stop_kl;
    // taken < nsched always holds in a trainer (taken <= j < S); the test
    // keeps a stray control block from indexing past the table
    const bool skip = stopped_in || trip || taken >= (uint32_t)a.nsched;
    float step_size = 0.f, bc2_sqrt = 1.f;
    if (!skip) {
        if (a.adaptive) {
            if (kl > a.kl_high) {
                lr = fmaxf(lr / 1.5f, a.lr_min);
            } else if (kl > 0.f && kl < a.kl_low) {
                lr = fminf(lr * 1.5f, a.lr_max);
            }
        }
        const float s0 = a.sched[2 * taken];
        bc2_sqrt = a.sched[2 * taken + 1];
        step_size = a.adaptive ? lr * s0 : s0;
    }
    // total squared norm, as clip_adam_kernel
    __shared__ double ssum[kBlock];
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += kBlock) s += part[b];
    ssum[threadIdx.x] = s;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) ssum[threadIdx.x] += ssum[threadIdx.x + h];
        __syncthreads();
    }
    const float total = (float)sqrt(ssum[0]);
    float c = max_norm / (total + 1e-6f);
    c = c < 1.0f ? c : 1.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (norm_out) *norm_out = total;
        a.slot_out[0] = (stopped_in || trip) ? 1u : 0u;
        a.slot_out[1] = skip ? taken : taken + 1u;
        a.slot_out[2] = __float_as_uint(lr);
        a.slot_out[3] = 0u;
    }
    if (skip) return;       // p, m, v untouched; g as the finish left it
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kBlock) {
        const float gi = (g[i] * gscale) * c;
        g[i] = gi;
        float mi = m[i];
        mi = mi + w1 * (gi - mi);
        float vi = v[i] * beta2 + (one_m_b2 * gi) * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = p[i] + (-step_size) * (mi / denom);
    }
}

int kl_check_gate(const dr_kl_gate *k, const char *who, KlGateArgs &a) {
    const std::string w(who);
    if (!k) return fail0(DR_ERR_INVALID, w + ": null gate");
    if (!k->control || (((uintptr_t)k->control) & 15))
        return fail0(DR_ERR_INVALID, w + ": control must be 16-byte aligned");
    if (k->num_steps < 1 || k->num_steps > INT32_MAX || k->step < 0 || k->step >= k->num_steps)
        return fail0(DR_ERR_INVALID, w + ": need 0 <= step < num_steps");
    if (!k->kl || !k->sched || (((uintptr_t)k->sched) & 7))
        return fail0(DR_ERR_INVALID, w + ": kl and sched (8-byte aligned) are required");
    if (!(k->stop_kl >= 0.0f) || !std::isfinite(k->stop_kl))
        return fail0(DR_ERR_INVALID, w + ": stop_kl must be finite and >= 0 (0 = no target)");
    if (k->adaptive != 0 && k->adaptive != 1)
        return fail0(DR_ERR_INVALID, w + ": adaptive must be 0 or 1");
    if (k->adaptive) {
        if (!(k->kl_low > 0.0f) || !(k->kl_high >= k->kl_low) || !std::isfinite(k->kl_high))
            return fail0(DR_ERR_INVALID, w + ": need 0 < kl_low <= kl_high, finite");
        if (!(k->lr_min > 0.0f) || !(k->lr_max >= k->lr_min) || !std::isfinite(k->lr_max))
            return fail0(DR_ERR_INVALID, w + ": need 0 < lr_min <= lr_max, finite");
    }
    const uint32_t *slots = static_cast<const uint32_t *>(k->control);
    a.slot_in = slots + 4 * k->step;
    a.slot_out = const_cast<uint32_t *>(slots) + 4 * (k->step + 1);
    a.kl = k->kl;
    a.sched = k->sched;
    a.nsched = (int)k->num_steps;
    a.has_target = k->stop_kl > 0.0f;
    a.adaptive = k->adaptive;
    a.stop_kl = k->stop_kl;
    a.kl_high = k->kl_high;
    a.kl_low = k->kl_low;
    a.lr_min = k->lr_min;
    a.lr_max = k->lr_max;
    return DR_OK;
}

int launch_adam_kl(int64_t n, float *params, float *grads, float *exp_avg, float *exp_avg_sq,
                   double beta1, double beta2, double eps, float max_grad_norm,
                   float *grad_norm_out, const float *sq_part, int nsq, hipStream_t st,
                   const char *who, const KlGateArgs &a) {
    // the scalars launch_adam forms, formed the same way
    const double b1 = beta1, b2 = beta2;
    hipLaunchKernelGGL(clip_adam_kl_kernel, dim3(nblocks_stream(n)), dim3(kBlock), 0, st, n,
                       params, grads, exp_avg, exp_avg_sq, sq_part, nsq, max_grad_norm,
                       (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps,
                       grad_norm_out, 1.0f, a);
    return check_launch(who);
}

}  // namespace
}  // namespace dr

extern "C" {

int dr_clip_adam_kl(int64_t n, float *params, float *grads, float *exp_avg, float *exp_avg_sq,
                    double beta1, double beta2, double eps, float max_grad_norm,
                    const dr_kl_gate *gate, float *grad_norm_out, void *workspace,
                    size_t workspace_bytes, void *stream) {
    if (n < 1 || !params || !grads || !exp_avg || !exp_avg_sq)
        return fail0(DR_ERR_INVALID, "dr_clip_adam_kl: bad arguments");
    KlGateArgs a{};
    int rc = kl_check_gate(gate, "dr_clip_adam_kl", a);
    if (rc) return rc;
    if (!workspace || workspace_bytes < dr_adam_workspace_bytes(n))
        return fail0(DR_ERR_INVALID, "dr_clip_adam_kl: workspace too small");
    const int nb = nblocks_stream(n);
    float *part = static_cast<float *>(workspace);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(kBlock), 0, st, n, grads, part, 1.0f);
    rc = check_launch("dr_clip_adam_kl norm");
    if (rc) return rc;
    return launch_adam_kl(n, params, grads, exp_avg, exp_avg_sq, beta1, beta2, eps,
                          max_grad_norm, grad_norm_out, part, nb, st, "dr_clip_adam_kl", a);
}

int dr_grad_finish_clip_adam_kl(const dr_grad_finish *f, int64_t n, float *params, float *grads,
                                float *exp_avg, float *exp_avg_sq, double beta1, double beta2,
                                double eps, float max_grad_norm, const dr_kl_gate *gate,
                                float *grad_norm_out, void *workspace, size_t workspace_bytes,
                                void *stream) {
    if (!f || n < 1 || !params || !grads || !exp_avg || !exp_avg_sq)
        return fail0(DR_ERR_INVALID, "dr_grad_finish_clip_adam_kl: bad arguments");
    KlGateArgs a{};
    int rc = kl_check_gate(gate, "dr_grad_finish_clip_adam_kl", a);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    int nb = 0;
    rc = launch_grad_finish(f, workspace, workspace_bytes, st, &nb);
    if (rc) return rc;
    return launch_adam_kl(n, params, grads, exp_avg, exp_avg_sq, beta1, beta2, eps,
                          max_grad_norm, grad_norm_out, static_cast<const float *>(workspace), nb,
                          st, "dr_grad_finish_clip_adam_kl", a);
}

}  // extern "C"
