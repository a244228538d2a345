// ed25519_probe.hip — the op table of ed25519_ops.h on the device: one lane
// per case.  Built into zelana_amd/libzkmi_edprobe.so for
// tests/test_gpu_ed25519.py (ctypes); nothing of libzkmi.so is linked or
// included, and the zelana_amd package never loads it.
#include <hip/hip_runtime.h>

#include "ed25519_ops.h"

using namespace edops;

// in: n x ED_IN words, out: n x ED_OUT words, nout[i] = words written (-1: refused)
__global__ void __launch_bounds__(64) ed_kernel(const uint32_t* __restrict__ ops, const uint32_t* __restrict__ in,
                                                uint32_t* __restrict__ out, int* __restrict__ nout, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  nout[i] = ed_apply(ops[i], in + (size_t)i * ED_IN, out + (size_t)i * ED_OUT);
}

extern "C" {
// allocate, copy in, launch (64-lane blocks), copy out, free; the first HIP
// error is returned, never aborted on
int ed_probe_run(int n, const uint32_t* ops, const uint32_t* in, uint32_t* out, int* nout) {
  if (n <= 0) return 0;
  const size_t nin = (size_t)n * ED_IN * 4, no = (size_t)n * ED_OUT * 4;
  uint32_t *dops = nullptr, *din = nullptr, *dout = nullptr;
  int* dn = nullptr;
  hipError_t e = hipMalloc(&dops, (size_t)n * 4);
  if (e == hipSuccess) e = hipMalloc(&din, nin);
  if (e == hipSuccess) e = hipMalloc(&dout, no);
  if (e == hipSuccess) e = hipMalloc(&dn, (size_t)n * 4);
  if (e == hipSuccess) e = hipMemcpy(dops, ops, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(din, in, nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, no);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ed_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, dops, din, dout, dn, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, no, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(nout, dn, (size_t)n * 4, hipMemcpyDeviceToHost);
  (void)hipFree(dops);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dn);
  return (int)e;
}
int ed_probe_words(int which) { return which ? ED_OUT : ED_IN; }
}
