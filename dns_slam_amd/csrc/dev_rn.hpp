// Single-rounding products and sums for code that must give the same bits in every translation unit: DNS_FMUL, DNS_FADD, DNS_FSUB,
// DNS_FDIV, DNS_DMUL, DNS_DADD.  Users: dev_sample.hpp (ray directions, far clip, sample depths), dev_encode.hpp (grid_cell) and
// track_fused.inc (pts = o + d z).
// By default they are the intrinsics __fmul_rn ... as ever.  Measured: with this toolchain's headers those are inline
// functions around the plain operators, compiled under the INCLUDING unit's -ffp-contract setting.  sample.hip and encode.hip are
// built with -ffp-contract=off; the fused tracker's units are not (their MLP bodies must round as mlp_split.hip's), and there
// dir . R, o + d z, farc tv + a and x s + 0.5 fuse: a ray direction one ulp off moves the far clip and with it a third of a draw's
// uniform samples by an ulp, a fused x s + 0.5 moves a grid cell's fraction, against sample.hip / encode.hip and the oracle.
// DNS_RN_NO_CONTRACT, defined by the fused tracker's stem form ahead of its includes, makes them functions that carry the setting
// themselves.  The non-stem fused units keep the intrinsics: they compile to what they were.
#pragma once
#include "common.hpp"
#ifdef DNS_RN_NO_CONTRACT
namespace dns {
namespace rn {
#define DNS_RN_OP(name, T, op)                                 \
  __device__ __forceinline__ T name(T a, T b) {                \
    _Pragma("clang fp contract(off)") return a op b;           \
  }
DNS_RN_OP(fmul, float, *)
DNS_RN_OP(fadd, float, +)
DNS_RN_OP(fsub, float, -)
DNS_RN_OP(fdiv, float, /)
DNS_RN_OP(dmul, double, *)
DNS_RN_OP(dadd, double, +)
#undef DNS_RN_OP
}  // namespace rn
}  // namespace dns
#define DNS_FMUL ::dns::rn::fmul
#define DNS_FADD ::dns::rn::fadd
#define DNS_FSUB ::dns::rn::fsub
#define DNS_FDIV ::dns::rn::fdiv
#define DNS_DMUL ::dns::rn::dmul
#define DNS_DADD ::dns::rn::dadd
#else
#define DNS_FMUL __fmul_rn
#define DNS_FADD __fadd_rn
#define DNS_FSUB __fsub_rn
#define DNS_FDIV __fdiv_rn
#define DNS_DMUL __dmul_rn
#define DNS_DADD __dadd_rn
#endif
