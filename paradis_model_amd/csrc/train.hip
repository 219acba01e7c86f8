// Rows f1-f3 of SURVEY.md section 8 (the callers right after / around the model in the training step):
//   f1  ParadisLoss forward + gradient in one pass   (reference utils/loss.py:233-282)
//   f2  rollout glue: strided channel-block copies that assemble the model input and the next
//       autoregressive input                          (reference trainer.py:534-538, 710-729)
//   f3  AdamW update, torch.optim.AdamW operation order (reference trainer.py:327-335)
// All HBM-bound streaming kernels.
#include <algorithm>
#include "common.h"
#include "stream_common.h"

namespace {

// per element:  l = wf[c] * wl[h] * loss(pred - target);  grad = wf*wl*loss'(e) / N
// kind 0 = mse, 1 = smooth reversed Huber with threshold delta.  partial[block] = sum of l.
__global__ void __launch_bounds__(256)
paradis_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                    const float* __restrict__ wf, const float* __restrict__ wl,
                    float* __restrict__ grad, float* __restrict__ partial, int C, int H, int W,
                    int64_t total, int kind, float delta, float inv_n) {
  __shared__ float red[4];
  float acc = 0.f;
  const int HW = H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int hw = (int)(i % HW);
    const int c = (int)((i / HW) % C);
    const int h = hw / W;
    const float wgt = wf[c] * (wl ? wl[h] : 1.0f);
    const float e = pred[i] - target[i];
    float l, dl;
    if (kind == 0) {
      l = e * e;
      dl = 2.0f * e;
    } else {
      const float a = fabsf(e);
      const float s = 1.0f / (1.0f + expf(-2.0f * (a - delta)));
      const float small = delta * a;
      const float large = (e * e + delta * delta) / (2.0f * delta);
      l = (1.0f - s) * small + s * large;
      const float ds = 2.0f * s * (1.0f - s);
      const float dla = ds * (large - small) + (1.0f - s) * delta + s * a / delta;
      dl = e > 0.f ? dla : (e < 0.f ? -dla : 0.f);
    }
    acc += l * wgt;
    if (grad) grad[i] = dl * wgt * inv_n;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256)
loss_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, int n, float inv_n) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += (double)partial[i];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)((red[0] + red[1] + red[2] + red[3]) * (double)inv_n);
}

__global__ void __launch_bounds__(256)
scale_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ y, int64_t n) {
  const float k = s[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[i] = x[i] * k;
}

// dst[b, c, :] = src[b, c, :] for c < C: batch strides differ (channel-block copy)
__global__ void __launch_bounds__(256)
copy_channels_kernel(const float* __restrict__ src, int64_t src_bs, float* __restrict__ dst,
                     int64_t dst_bs, int B, int64_t per /* C*P */) {
  const int64_t total = (int64_t)B * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / per, r = i - b * per;
    dst[b * dst_bs + r] = src[b * src_bs + r];
  }
}

// torch.optim.AdamW, same operation order as the ATen implementation:
//   p *= 1 - lr*wd;  m = lerp(m, g, 1-b1);  v = b2*v + (1-b2)*g*g;
//   denom = sqrt(v)/sqrt(bc2) + eps;  p -= (lr/bc1) * m / denom
// The scalar coefficients are what torch hands its fp32 kernels: formed in DOUBLE from the double hyper-parameters and
// rounded once (1 - 0.9 -> 0.1f).  Formed in fp32 from fp32-rounded betas, 1.0f - 0.9f = 0.10000002 is 2.4e-7 off, and so
// were m and v after every step (tests/test_hip_kernel_edges.py::test_adamw).
struct AdamWCoef { float decay, omb1, b2, omb2, eps, step_size, bc2_sqrt; };

AdamWCoef adamw_coef(double lr, double b1, double b2, double eps, double wd, int step) {
  const int st = step >= 1 ? step : 1;
  lr = (double)(float)lr;     // the device-state path holds lr as fp32 bits: both paths form the same coefficients, bit for bit
  AdamWCoef k;
  k.decay = (float)(1.0 - lr * wd);
  k.omb1 = (float)(1.0 - b1);
  k.b2 = (float)b2;
  k.omb2 = (float)(1.0 - b2);
  k.eps = (float)eps;
  k.step_size = (float)(lr / (1.0 - pow(b1, st)));
  k.bc2_sqrt = (float)sqrt(1.0 - pow(b2, st));
  return k;
}

__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, int64_t i, const AdamWCoef& k) {
  const float gi = g[i];
  float pi = p[i] * k.decay;
  float mi = m[i];
  mi = mi + k.omb1 * (gi - mi);
  const float vi = k.b2 * v[i] + k.omb2 * gi * gi;
  const float denom = sqrtf(vi) / k.bc2_sqrt + k.eps;
  pi = pi - k.step_size * (mi / denom);
  p[i] = pi; m[i] = mi; v[i] = vi;
}

__global__ void __launch_bounds__(256)
adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
             float* __restrict__ v, int64_t n, AdamWCoef k) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    adamw_update(p, g, m, v, i, k);
}

// One launch for a whole parameter group: block c works on chunk c = (tensor index, offset); all
// tensors share the hyper-parameters and the step count.  (335 per-tensor launches of ~5 us are
// launch-bound: 0.7 % of the training step.)  The chunk table: stream_common.h.
// dev (optional): {int32 step at [0], the bits of the fp32 lr at [1]} kept on the device so
// that a captured HIP graph of the training step stays valid from one replay to the next (the host-side step
// count and learning rate would be frozen into the kernel arguments): the coefficients that depend on them are then
// formed here, in double like the host path.
__global__ void __launch_bounds__(256)
adamw_multi_kernel(const int64_t* __restrict__ ptrs /* [4][T]: p, g, m, v */, const int64_t* __restrict__ numel,
                   const int* __restrict__ chunk_tensor, const int64_t* __restrict__ chunk_off, int T,
                   AdamWCoef k, double b1, double b2, double wd, const int* __restrict__ dev) {
  if (dev) {     // (workgroup-uniform)
    // one thread forms the coefficients (two double pow + a sqrt), the workgroup reads them from LDS.  Same formulas
    // in double as the host path; the device's pow is not guaranteed to round like the host's libm, so the two paths
    // agree to ~1 ulp of the fp32 coefficients, not bit for bit (tests/test_hip_train_rows.py checks 1e-6).
    __shared__ float co[3];
    if (threadIdx.x == 0) {
      const int step = dev[0];
      const double lr = (double)__int_as_float(dev[1]);
      co[0] = (float)(1.0 - lr * wd);
      co[1] = (float)(lr / (1.0 - pow(b1, (double)step)));
      co[2] = (float)sqrt(1.0 - pow(b2, (double)step));
    }
    __syncthreads();
    k.decay = co[0];
    k.step_size = co[1];
    k.bc2_sqrt = co[2];
  }
  const TableChunk c = table_chunk(numel, chunk_tensor, chunk_off, T);
  if (c.n == 0) return;       // (workgroup-uniform) a bad table entry touches nothing
  float* p = reinterpret_cast<float*>(ptrs[c.t]) + c.off;
  const float* g = reinterpret_cast<const float*>(ptrs[T + c.t]) + c.off;
  float* m = reinterpret_cast<float*>(ptrs[2 * T + c.t]) + c.off;
  float* v = reinterpret_cast<float*>(ptrs[3 * T + c.t]) + c.off;
  for (int64_t i = threadIdx.x; i < c.n; i += 256) adamw_update(p, g, m, v, i, k);
}

__global__ void adamw_tick_kernel(int* __restrict__ dev) { dev[0] += 1; }

// thread g: the learning rate of group g for its (already ticked, 1-based) step count, out of row g of the table;
// past the end of the table the last entry holds.  An address of 0 = a group without a device state.
__global__ void __launch_bounds__(64)
lr_schedule_kernel(const int64_t* __restrict__ states, const float* __restrict__ table, int G, int n) {
  for (int g = threadIdx.x; g < G; g += 64) {
    int* st = reinterpret_cast<int*>(states[g]);
    if (st == nullptr) continue;
    const int k = min(max(st[0] - 1, 0), n - 1);
    st[1] = __float_as_int(table[(int64_t)g * n + k]);
  }
}

inline int blocks_for(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 8));
}

}  // namespace

extern "C" int paradis_loss_blocks(int64_t total) { return blocks_for(total); }

extern "C" int paradis_loss_fwd_bwd(const float* pred, const float* target, const float* wf,
                                    const float* wl, float* loss, float* grad, float* partial, int B,
                                    int C, int H, int W, int kind, float delta, void* stream) {
  PD_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "loss_fwd_bwd: bad shape");
  PD_REQUIRE(kind == 0 || kind == 1, "loss_fwd_bwd: kind must be 0 (mse) or 1 (reversed_huber)");
  PD_REQUIRE(partial != nullptr && loss != nullptr, "loss_fwd_bwd: workspace/result missing");
  const int64_t total = (int64_t)B * C * H * W;
  const int nb = blocks_for(total);
  const float inv_n = (float)(1.0 / (double)total);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(paradis_loss_kernel, dim3(nb), dim3(256), 0, st, pred, target, wf, wl, grad, partial, C,
                     H, W, total, kind, delta, inv_n);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, partial, loss, nb, inv_n);
  PD_CHECK_LAUNCH("loss_fwd_bwd");
  return 0;
}

extern "C" int paradis_scale(const float* x, const float* scalar, float* y, int64_t n, void* stream) {
  PD_REQUIRE(n >= 0, "scale: bad size");
  if (n == 0) return 0;
  hipLaunchKernelGGL(scale_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, x, scalar, y, n);
  PD_CHECK_LAUNCH("scale");
  return 0;
}

extern "C" int paradis_copy_channels(const float* src, int64_t src_bs, float* dst, int64_t dst_bs, int B,
                                     int64_t per_sample, void* stream) {
  PD_REQUIRE(B >= 0 && per_sample >= 0, "copy_channels: bad size");
  if (B == 0 || per_sample == 0) return 0;
  hipLaunchKernelGGL(copy_channels_kernel, dim3(blocks_for((int64_t)B * per_sample)), dim3(256), 0,
                     (hipStream_t)stream, src, src_bs, dst, dst_bs, B, per_sample);
  PD_CHECK_LAUNCH("copy_channels");
  return 0;
}

extern "C" int paradis_adamw_chunk(void) { return TABLE_CHUNK; }

extern "C" int paradis_adamw_multi_d(const int64_t* ptrs, const int64_t* numel, const int* chunk_tensor,
                                     const int64_t* chunk_off, int n_tensors, int n_chunks, double lr,
                                     double beta1, double beta2, double eps, double weight_decay, int step,
                                     const int* dev_state, void* stream) {
  PD_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && (step >= 1 || dev_state != nullptr), "adamw_multi: bad arguments");
  if (n_chunks == 0) return 0;
  PD_REQUIRE(ptrs && numel && chunk_tensor && chunk_off, "adamw_multi: tables missing");
  hipLaunchKernelGGL(adamw_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, ptrs, numel,
                     chunk_tensor, chunk_off, n_tensors, adamw_coef(lr, beta1, beta2, eps, weight_decay, step), beta1,
                     beta2, weight_decay, dev_state);
  PD_CHECK_LAUNCH("adamw_multi");
  return 0;
}

extern "C" int paradis_adamw_multi(const int64_t* ptrs, const int64_t* numel, const int* chunk_tensor,
                                   const int64_t* chunk_off, int n_tensors, int n_chunks, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int step,
                                   const int* dev_state, void* stream) {
  return paradis_adamw_multi_d(ptrs, numel, chunk_tensor, chunk_off, n_tensors, n_chunks, lr, beta1, beta2, eps,
                               weight_decay, step, dev_state, stream);
}

// dev_state[0] += 1 on the stream (the step count of a captured training step lives on the device)
extern "C" int paradis_adamw_tick(int* dev_state, void* stream) {
  PD_REQUIRE(dev_state != nullptr, "adamw_tick: state missing");
  hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, dev_state);
  PD_CHECK_LAUNCH("adamw_tick");
  return 0;
}

// states[g] (DEVICE table of n_groups addresses, 0 = skip) -> int32[2] state of group g; table [n_groups][n_steps] fp32
// on the device: state_g[1] = bits(table[g][min(state_g[0] - 1, n_steps - 1)]).  One launch of one wavefront.
extern "C" int paradis_lr_schedule(const int64_t* states, const float* table, int n_groups, int n_steps, void* stream) {
  PD_REQUIRE(n_groups >= 0 && n_steps >= 1, "lr_schedule: bad arguments");
  if (n_groups == 0) return 0;
  PD_REQUIRE(states != nullptr && table != nullptr, "lr_schedule: tables missing");
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, states, table, n_groups, n_steps);
  PD_CHECK_LAUNCH("lr_schedule");
  return 0;
}

extern "C" int paradis_adamw_step_d(float* p, const float* g, float* m, float* v, int64_t n, double lr,
                                    double beta1, double beta2, double eps, double weight_decay, int step,
                                    void* stream) {
  PD_REQUIRE(n >= 0 && step >= 1, "adamw_step: bad arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                     adamw_coef(lr, beta1, beta2, eps, weight_decay, step));
  PD_CHECK_LAUNCH("adamw_step");
  return 0;
}

extern "C" int paradis_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int step,
                                  void* stream) {
  return paradis_adamw_step_d(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, stream);
}
