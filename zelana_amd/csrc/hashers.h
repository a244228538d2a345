// hashers.h — the two resident hashers as every store that hashes with them
// sees them (note_tree.hip, account_tree.hip, note_scan.hip),
// and the host steps their entry points share.  Internal to libzkmi.so.
#pragma once
#include <vector>

#include "mimc_hash.h"
#include "poseidon_hash.h"
#include "zkmi_internal.h"

struct zkmi_mimc {
  zkmi_ctx* ctx = nullptr;
  zk::Fe table[zk::MIMC_NTABLE];  // host copy (the empty-subtree chain is made on the host)
  zk::Fe* d_table = nullptr;
  ~zkmi_mimc() {
    if (d_table) (void)hipFree(d_table);
  }
};

struct zkmi_poseidon {
  zkmi_ctx* ctx = nullptr;
  uint32_t half = 0, rounds = 0, nconst = 0;
  std::vector<zk::Fe> table;  // Montgomery form, host copy (the empty-subtree chain is made on the host)
  // the quad mapping for launches of few hashes; off with ZKMI_DEBUG_NOTE_TREE_NO_QUAD=1
  // at create (every launch then runs one lane per hash: tools/note_tree.py's A/B)
  bool quad = true;
  zk::Fe* d_table = nullptr;
  ~zkmi_poseidon() {
    if (d_table) (void)hipFree(d_table);
  }
};

namespace zk {

// The tail of a hasher's create: its table of n constants into a device
// buffer of its own (*d_table, which the hasher's destructor frees).  0, or
// the error code with the message set under the entry point's name fn; the
// caller deletes the hasher on failure.
inline int hasher_upload_table(const char* fn, zkmi_ctx* ctx, const Fe* table, size_t n, Fe** d_table) {
  if (hipMalloc((void**)d_table, n * sizeof(Fe)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: hipMalloc failed", fn);
    return ZKMI_ENOMEM;
  }
  hipError_t e = hipMemcpyAsync(*d_table, table, n * sizeof(Fe), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    set_error("%s: upload failed (%s)", fn, hipGetErrorString(e));
    return ZKMI_EHIP;
  }
  return 0;
}

// The round trip of a hash_many: n tuples of `arity` elements into the
// workspace buffer ws_in, launch(d_in, d_out) under the kernel timer `timer`,
// the n hashes back from ws_out.  Returns with the results on the host.
template <class Launch>
int hasher_hash_many(zkmi_ctx* ctx, const char* ws_in, const char* ws_out, const char* timer, size_t n, uint32_t arity,
                     const uint64_t* in, uint64_t* out, Launch launch) {
  uint32_t *d_in, *d_out;
  ZK_TRY(ctx->ws.get(ws_in, n * arity * 32, (void**)&d_in));
  ZK_TRY(ctx->ws.get(ws_out, n * 32, (void**)&d_out));
  ZK_HIP(hipMemcpyAsync(d_in, in, n * arity * 32, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, timer);
    launch(d_in, d_out);
  }
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(out, d_out, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return timer_flush(ctx);
}

}  // namespace zk
