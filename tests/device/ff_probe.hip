// ff_probe.hip — the op table of ff_ops.h on the device: one lane per case,
// the op a uniform kernel argument.  Built into zelana_amd/libzkmi_ffprobe.so
// for tests/test_gpu_ff_ops.py (ctypes); nothing of libzkmi.so is linked or
// included, and the zelana_amd package never loads it.
#include <hip/hip_runtime.h>

#include "ff_ops.h"

using namespace ffops;

template <class P>
__global__ void __launch_bounds__(64) field_kernel(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                   uint32_t* __restrict__ flag, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe a[N_IN], r[N_OUT];
  for (int s = 0; s < N_IN; s++)
    for (int l = 0; l < NL; l++) a[s].v[l] = in[((size_t)i * N_IN + s) * NL + l];
  for (int s = 0; s < N_OUT; s++)
    for (int l = 0; l < NL; l++) r[s].v[l] = out[((size_t)i * N_OUT + s) * NL + l];
  uint32_t f = flag[i];
  field_apply<P>(op, a, r, &f);
  for (int s = 0; s < N_OUT; s++)
    for (int l = 0; l < NL; l++) out[((size_t)i * N_OUT + s) * NL + l] = r[s].v[l];
  flag[i] = f;
}

template <class F>
__global__ void __launch_bounds__(64) curve_kernel(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                   uint32_t* __restrict__ flag, int n) {
  using T = typename F::T;
  constexpr int W = sizeof(T) / sizeof(uint32_t);  // 9 (Fe) or 18 (Fe2: c0 then c1)
  static_assert(sizeof(T) == W * sizeof(uint32_t), "coordinates are plain limb arrays");
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T a[N_IN], r[N_OUT];
  for (int s = 0; s < N_IN; s++) {
    uint32_t* d = reinterpret_cast<uint32_t*>(&a[s]);
    for (int l = 0; l < W; l++) d[l] = in[((size_t)i * N_IN + s) * W + l];
  }
  uint32_t f = flag[i];
  curve_apply<F>(op, a, r, &f);
  for (int s = 0; s < N_OUT; s++) {
    const uint32_t* d = reinterpret_cast<const uint32_t*>(&r[s]);
    for (int l = 0; l < W; l++) out[((size_t)i * N_OUT + s) * W + l] = d[l];
  }
  flag[i] = f;
}

// allocate, copy in, launch (64-lane blocks), copy out, free; the first HIP
// error is returned, never aborted on.  width: u32 words per slot.
template <class K>
static int run(K kernel, int op, const uint32_t* in, uint32_t* out, uint32_t* flag, int n, int width) {
  if (n <= 0) return 0;
  const size_t nin = (size_t)n * N_IN * width * 4, nout = (size_t)n * N_OUT * width * 4, nfl = (size_t)n * 4;
  uint32_t *din = nullptr, *dout = nullptr, *dfl = nullptr;
  hipError_t e = hipMalloc(&din, nin);
  if (e == hipSuccess) e = hipMalloc(&dout, nout);
  if (e == hipSuccess) e = hipMalloc(&dfl, nfl);
  if (e == hipSuccess) e = hipMemcpy(din, in, nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dout, out, nout, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dfl, flag, nfl, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, 0, op, din, dout, dfl, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, nout, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flag, dfl, nfl, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dfl);
  return (int)e;
}

extern "C" {
// field: 0 FqP, 1 FrP, 2 FqPn.  in: n x 8 x 9, out: n x 4 x 9, flag: n (u32).
// Returns the HIP error code, or -1 for an op the field does not have.
int ff_probe_field(int field, int op, const uint32_t* in, uint32_t* out, uint32_t* flag, int n) {
  switch (field) {
    case 0: return field_op_supported<FqP>(op) ? run(field_kernel<FqP>, op, in, out, flag, n, NL) : -1;
    case 1: return field_op_supported<FrP>(op) ? run(field_kernel<FrP>, op, in, out, flag, n, NL) : -1;
    case 2: return field_op_supported<FqPn>(op) ? run(field_kernel<FqPn>, op, in, out, flag, n, NL) : -1;
    default: return -1;
  }
}
// group: 0 G1 (FqOps, 9 words a slot), 1 G2 (Fq2Ops, 18 words a slot)
int ff_probe_curve(int group, int op, const uint32_t* in, uint32_t* out, uint32_t* flag, int n) {
  switch (group) {
    case 0: return curve_op_supported<FqOps>(op) ? run(curve_kernel<FqOps>, op, in, out, flag, n, NL) : -1;
    case 1: return curve_op_supported<Fq2Ops>(op) ? run(curve_kernel<Fq2Ops>, op, in, out, flag, n, 2 * NL) : -1;
    default: return -1;
  }
}
}
