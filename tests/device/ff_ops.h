// ff_ops.h — one table of the ff.h / ec.h routines, compiled for the host
// (tests/native/ff_host_shim.cpp) and for the device (ff_probe.hip), so both
// builds of the same integer program can be compared per op with the integer
// model in tests/ff_model.py.  Host+device, no HIP calls.
//
// Slots are raw elements (Fe: 9 x u32 limbs, not the packed form), so a case
// can hand in unnormalised limbs.  Field ops: 8 input Fe, 4 output Fe and one
// flag word per case.  Curve ops: 8 input and 4 output coordinates (Fe for
// G1, Fe2 for G2): P in slots 0..3 (x, y, zz, zzz; an affine P uses 0, 1), Q
// in slots 4..7, the result in the four outputs.  The flag word is an input
// for fq_cneg and an output for is_zero, eq and xyzz_madd_g1f's *inf.
// The op ids are mirrored by name in tests/ff_model.py (FIELD_OPS, CURVE_OPS).
#pragma once
#include <type_traits>

#include "../../zelana_amd/csrc/ec.h"

namespace ffops {
using namespace zk;

constexpr int N_IN = 8, N_OUT = 4;

enum FieldOp : int {
  F_MUL, F_SQR, F_MUL_ADD, F_SQR_ADD, F_MUL2, F_MUL4, F_MUL_X2, F_SQR_X2,
  F_ADD, F_SUB, F_DBL, F_NEG, F_ADD_LAZY, F_SUBK2, F_SUBK4, F_SUBK6, F_SUBK8,
  F_REDUCE_Q32, F_REDUCE, F_IS_ZERO, F_EQ, F_TO_MONT, F_FROM_MONT, F_PACK_UNPACK,
  F_BSUB_B2_1, F_BSUB_B4_1, F_BSUB_B8_1, F_BSUB_B10_1, F_BSUB2_B6_3, F_BSUBADD_B10_1,
  F_FQ_CNEG, F_F2_MUL, F_F2_SQR, F_F2_MUL_N, F_F2_SQR_N, F_COUNT
};
enum CurveOp : int {
  C_MADD_G1, C_MADD_G1F, C_MMADD_G1, C_ADD_G1, C_MADD_G2, C_MMADD_G2, C_ADD_G2,
  C_MDBL, C_DBL, C_MADD, C_ADD, C_COUNT
};

// which ops exist for which field parameter: the interleaved pairs are
// written on the inline-asm mads (FqP, FrP), the borrow forms and fq_cneg on
// FqP's constants, Fq2 on FqPn
template <class P>
ZK_HD bool field_op_supported(int op) {
  if (op < 0 || op >= F_COUNT) return false;
  if (op == F_MUL_X2 || op == F_SQR_X2) return !std::is_same<P, FqPn>::value;
  if (op >= F_BSUB_B2_1 && op <= F_FQ_CNEG) return std::is_same<P, FqP>::value;
  if (op >= F_F2_MUL) return std::is_same<P, FqPn>::value;
  return true;
}
template <class F>
ZK_HD bool curve_op_supported(int op) {
  if (op < 0 || op >= C_COUNT) return false;
  if (op <= C_ADD_G1) return std::is_same<F, FqOps>::value;
  if (op <= C_ADD_G2) return std::is_same<F, Fq2Ops>::value;
  return true;
}

template <class P>
ZK_HD void field_apply(int op, const Fe* in, Fe* out, uint32_t* flag) {
  switch (op) {
    case F_MUL: out[0] = mul<P>(in[0], in[1]); break;
    case F_SQR: out[0] = sqr<P>(in[0]); break;
    case F_MUL_ADD: out[0] = mul_add<P>(in[0], in[1], in[2]); break;
    case F_SQR_ADD: out[0] = sqr_add<P>(in[0], in[1]); break;
    case F_MUL2: out[0] = mul2<P>(in[0], in[1], in[2], in[3]); break;
    case F_MUL4: out[0] = mul4<P>(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7]); break;
    case F_ADD: out[0] = add<P>(in[0], in[1]); break;
    case F_SUB: out[0] = sub<P>(in[0], in[1]); break;
    case F_DBL: out[0] = dbl<P>(in[0]); break;
    case F_NEG: out[0] = neg<P>(in[0]); break;
    case F_ADD_LAZY: out[0] = add_lazy(in[0], in[1]); break;
    case F_SUBK2: out[0] = subk<P, 2>(in[0], in[1]); break;
    case F_SUBK4: out[0] = subk<P, 4>(in[0], in[1]); break;
    case F_SUBK6: out[0] = subk<P, 6>(in[0], in[1]); break;
    case F_SUBK8: out[0] = subk<P, 8>(in[0], in[1]); break;
    case F_REDUCE_Q32: out[0] = reduce_q32<P>(in[0]); break;
    case F_REDUCE: out[0] = reduce<P>(in[0]); break;
    case F_IS_ZERO: *flag = is_zero<P>(in[0]) ? 1u : 0u; break;
    case F_EQ: *flag = eq<P>(in[0], in[1]) ? 1u : 0u; break;
    case F_TO_MONT: out[0] = to_mont<P>(in[0]); break;
    case F_FROM_MONT: out[0] = from_mont<P>(in[0]); break;
    case F_PACK_UNPACK: {
      uint32_t w[8];
      pack(w, in[0]);
      out[0] = unpack(w);
      break;
    }
    default: break;
  }
  if constexpr (!std::is_same<P, FqPn>::value) {
    if (op == F_MUL_X2) mul_x2<P>(in[0], in[1], in[2], in[3], out[0], out[1]);
    if (op == F_SQR_X2) sqr_x2<P>(in[0], in[1], out[0], out[1]);
  }
  if constexpr (std::is_same<P, FqP>::value) {
    switch (op) {
      case F_BSUB_B2_1: out[0] = bsub(FqP::B2_1, in[0]); break;
      case F_BSUB_B4_1: out[0] = bsub(FqP::B4_1, in[0]); break;
      case F_BSUB_B8_1: out[0] = bsub(FqP::B8_1, in[0]); break;
      case F_BSUB_B10_1: out[0] = bsub(FqP::B10_1, in[0]); break;
      case F_BSUB2_B6_3: out[0] = bsub2(FqP::B6_3, in[0], in[1]); break;
      case F_BSUBADD_B10_1: out[0] = bsubadd(FqP::B10_1, in[0], in[1]); break;
      case F_FQ_CNEG: out[0] = fq_cneg(in[0], *flag != 0); break;
      default: break;
    }
  }
  if constexpr (std::is_same<P, FqPn>::value) {
    Fe2 r;
    switch (op) {
      case F_F2_MUL: r = f2_mul(Fe2{in[0], in[1]}, Fe2{in[2], in[3]}); break;
      case F_F2_SQR: r = f2_sqr(Fe2{in[0], in[1]}); break;
      case F_F2_MUL_N: r = f2_mul_n(Fe2{in[0], in[1]}, Fe2{in[2], in[3]}); break;
      case F_F2_SQR_N: r = f2_sqr_n(Fe2{in[0], in[1]}); break;
      default: return;
    }
    out[0] = r.c0;
    out[1] = r.c1;
  }
}

template <class F>
ZK_HD void curve_apply(int op, const typename F::T* in, typename F::T* out, uint32_t* flag) {
  const Xyzz<F> p{in[0], in[1], in[2], in[3]}, q{in[4], in[5], in[6], in[7]};
  const Aff<F> pa{in[0], in[1]}, qa{in[4], in[5]};
  Xyzz<F> r = xyzz_inf<F>();
  if constexpr (std::is_same<F, FqOps>::value) {
    switch (op) {
      case C_MADD_G1: r = xyzz_madd_g1(p, qa); break;
      case C_MADD_G1F: {
        bool inf = false;
        r = xyzz_madd_g1f(p, qa.x, qa.y, &inf);
        *flag = inf ? 1u : 0u;
        break;
      }
      case C_MMADD_G1: r = xyzz_mmadd_g1(pa, qa); break;
      case C_ADD_G1: r = xyzz_add_g1(p, q); break;
      default: break;
    }
  } else {
    switch (op) {
      case C_MADD_G2: r = xyzz_madd_g2(p, qa); break;
      case C_MMADD_G2: r = xyzz_mmadd_g2(pa, qa); break;
      case C_ADD_G2: r = xyzz_add_g2(p, q); break;
      default: break;
    }
  }
  switch (op) {
    case C_MDBL: r = xyzz_mdbl(pa); break;
    case C_DBL: r = xyzz_dbl(p); break;
    case C_MADD: r = xyzz_madd(p, qa); break;
    case C_ADD: r = xyzz_add(p, q); break;
    default: break;
  }
  out[0] = r.x;
  out[1] = r.y;
  out[2] = r.zz;
  out[3] = r.zzz;
}

}  // namespace ffops
