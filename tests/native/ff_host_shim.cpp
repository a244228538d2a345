// Host build of zelana_amd/csrc/ff.h and ec.h (the exact source the gfx950
// kernels use): the op table of tests/device/ff_ops.h looped over on the CPU,
// so the limb arithmetic can be compared per op with Python integers
// (tests/test_ff_ops_cpu.py) and with the device build of the same table
// (tests/test_gpu_ff_ops.py).  Built into zelana_amd/libff_host.so.
#include <string.h>

#include "../device/ff_ops.h"

using namespace ffops;

template <class P>
static void field_loop(int op, const uint32_t* in, uint32_t* out, uint32_t* flag, int n) {
  for (int i = 0; i < n; i++) {
    Fe a[N_IN], r[N_OUT];
    memcpy(a, in + (size_t)i * N_IN * NL, sizeof a);
    memcpy(r, out + (size_t)i * N_OUT * NL, sizeof r);
    field_apply<P>(op, a, r, flag + i);
    memcpy(out + (size_t)i * N_OUT * NL, r, sizeof r);
  }
}
template <class F>
static void curve_loop(int op, const uint32_t* in, uint32_t* out, uint32_t* flag, int n) {
  using T = typename F::T;
  constexpr int W = sizeof(T) / sizeof(uint32_t);
  static_assert(sizeof(T) == W * sizeof(uint32_t), "coordinates are plain limb arrays");
  for (int i = 0; i < n; i++) {
    T a[N_IN], r[N_OUT];
    memcpy(a, in + (size_t)i * N_IN * W, sizeof a);
    curve_apply<F>(op, a, r, flag + i);
    memcpy(out + (size_t)i * N_OUT * W, r, sizeof r);
  }
}

extern "C" {
// the signatures of ff_probe.hip's entries; 0, or -1 for an op the field does not have
int ff_host_field(int field, int op, const uint32_t* in, uint32_t* out, uint32_t* flag, int n) {
  switch (field) {
    case 0: return field_op_supported<FqP>(op) ? (field_loop<FqP>(op, in, out, flag, n), 0) : -1;
    case 1: return field_op_supported<FrP>(op) ? (field_loop<FrP>(op, in, out, flag, n), 0) : -1;
    case 2: return field_op_supported<FqPn>(op) ? (field_loop<FqPn>(op, in, out, flag, n), 0) : -1;
    default: return -1;
  }
}
int ff_host_curve(int group, int op, const uint32_t* in, uint32_t* out, uint32_t* flag, int n) {
  switch (group) {
    case 0: return curve_op_supported<FqOps>(op) ? (curve_loop<FqOps>(op, in, out, flag, n), 0) : -1;
    case 1: return curve_op_supported<Fq2Ops>(op) ? (curve_loop<Fq2Ops>(op, in, out, flag, n), 0) : -1;
    default: return -1;
  }
}
}
