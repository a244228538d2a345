// tx_msg_probe.hip — the four message builders of zelana_amd/csrc/tx_msg.h on
// the device: one lane per case, each message through the 16-byte sink the
// kernels of tx_auth.hip use.  Built into zelana_amd/libzkmi_txprobe.so for
// tests/test_gpu_tx_auth.py (ctypes); nothing of libzkmi.so is linked or
// included, and the zelana_amd package never loads it.
#include <hip/hip_runtime.h>

#include "../../zelana_amd/csrc/tx_msg.h"

using namespace zk;

constexpr int TX_PROBE_IN = 22;  // words of a case: from, to, amount, nonce, chain_id (the first 88 bytes of a record)

// in: n x 22 words; out: n x 4 slots of TX_MSG_STRIDE bytes (readable
// transfer, readable withdrawal, legacy transfer, legacy withdrawal);
// lens: n x 4
__global__ void __launch_bounds__(64) tx_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                uint32_t* __restrict__ lens, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t r[TX_PROBE_IN];
#pragma unroll
  for (int w = 0; w < TX_PROBE_IN; w++) r[w] = in[(size_t)i * TX_PROBE_IN + w];
  const uint64_t amount = tx_rec_u64(r, 16), nonce = tx_rec_u64(r, 18), chain_id = tx_rec_u64(r, 20);
  uint32_t* slot = out + (size_t)i * 4 * (TX_MSG_STRIDE / 4);
  TxQuadSink s0{slot}, s1{slot + TX_MSG_STRIDE / 4}, s2{slot + 2 * (TX_MSG_STRIDE / 4)}, s3{slot + 3 * (TX_MSG_STRIDE / 4)};
  lens[4 * i] = tx_transfer_message(s0, r, r + 8, amount, nonce, chain_id);
  lens[4 * i + 1] = tx_withdraw_message(s1, r, r + 8, amount, nonce);
  lens[4 * i + 2] = tx_legacy_transfer_message(s2, r, r + 8, amount, nonce, chain_id);
  lens[4 * i + 3] = tx_legacy_withdraw_message(s3, r, r + 8, amount, nonce);
}

extern "C" {
// allocate, copy in, launch (64-lane blocks), copy out, free; the first HIP
// error is returned, never aborted on.  The slots are filled with 0xA5 first,
// so what a builder leaves unwritten shows.
int tx_probe_run(int n, const uint32_t* in, uint8_t* out, uint32_t* lens) {
  if (n <= 0) return 0;
  const size_t nin = (size_t)n * TX_PROBE_IN * 4, no = (size_t)n * 4 * TX_MSG_STRIDE, nl = (size_t)n * 16;
  uint32_t *din = nullptr, *dout = nullptr, *dl = nullptr;
  hipError_t e = hipMalloc(&din, nin);
  if (e == hipSuccess) e = hipMalloc(&dout, no);
  if (e == hipSuccess) e = hipMalloc(&dl, nl);
  if (e == hipSuccess) e = hipMemcpy(din, in, nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xA5, no);
  if (e == hipSuccess) e = hipMemset(dl, 0, nl);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(tx_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, din, dout, dl, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, no, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(lens, dl, nl, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dl);
  return (int)e;
}
int tx_probe_stride(void) { return (int)TX_MSG_STRIDE; }
}
