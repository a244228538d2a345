// r1cs_row.h — the row predicate of the R1CS satisfaction check (groth16.hip
// k_r1cs_scan), host + device so a host program can test it
// (tests/host/r1cs_row_check.cpp).
#pragma once
#include "ff.h"

namespace zk {

// a, b, c: <a_i,z>, <b_i,z>, <c_i,z> as k_matvec leaves them: value form (not
// Montgomery), normalised limbs, only reduced below 2r.  True when a b != c
// mod r.  mul<FrP> of two value-form numbers is a b R^-1 (< 2r); the product
// by R^2 brings it back to value form (as k_qap_combine), and eq<FrP> fully
// reduces both sides before it compares, so x and x + r are the same value.
ZK_HD bool r1cs_row_bad(const Fe& a, const Fe& b, const Fe& c) {
  const Fe ab = mul<FrP>(mul<FrP>(a, b), fe_const<FrP>(FrP::R2));
  return !eq<FrP>(ab, c);
}

}  // namespace zk
