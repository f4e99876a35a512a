// kr_point_dual.hpp - the physics of one grid point, y -> (y_s, z), on dual numbers: forward-mode automatic
// differentiation in fp64 (one tangent direction per evaluation).  Shared by the per-point derivative kernels
// (kr_vjp.hip: kr_ode_vjp_batch, kr_ode_jacobian_batch) and the step adjoint (kr_adj.hip: kr_step_vjp_batch,
// kr_simulate_vjp_batch), which all differentiate the same map - CosseratRodTorch.ODE_parallel (reference
// cosserat_ode_torch.py:264-306) with the MLP off.
#pragma once
#include "rod_device.hpp"

namespace kr {

struct Dual {
  double v, d;
};
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator-(Dual a) { return {-a.v, -a.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, fma(a.v, b.d, a.d * b.v)}; }
__device__ __forceinline__ Dual operator*(double s, Dual a) { return {s * a.v, s * a.d}; }
__device__ __forceinline__ Dual operator+(Dual a, double s) { return {a.v + s, a.d}; }
__device__ __forceinline__ Dual dual_rcp(Dual a) {
  const double r = 1.0 / a.v;
  return {r, -a.d * r * r};
}
__device__ __forceinline__ Dual dual_abs(Dual a) { return a.v < 0.0 ? Dual{-a.v, -a.d} : a; }  // (torch: sign(0) = 0; d = 0 then anyway for q = 0 ... kept as the value's sign)
__device__ __forceinline__ Dual detach(Dual a) { return {a.v, 0.0}; }
// a constant of the point map as a dual number: a plain one has no tangent, one that carries a tangent is itself
__device__ __forceinline__ Dual dual_of(double x) { return {x, 0.0}; }
__device__ __forceinline__ Dual dual_of(Dual x) { return x; }

// a plain value beside the dual numbers: what an input is when the tangent runs along the constants alone
__device__ __forceinline__ double dual_rcp(double a) { return 1.0 / a; }
__device__ __forceinline__ double dual_abs(double a) { return a < 0.0 ? -a : a; }
__device__ __forceinline__ double detach(double a) { return a; }
__device__ __forceinline__ Dual operator*(Dual a, double s) { return {a.v * s, a.d * s}; }
__device__ __forceinline__ Dual operator+(double s, Dual a) { return {s + a.v, a.d}; }
__device__ __forceinline__ Dual operator-(Dual a, double s) { return {a.v - s, a.d}; }
__device__ __forceinline__ Dual operator-(double s, Dual a) { return {s - a.v, -a.d}; }

// vectors and matrices of either kind; a mixed operation gives the kind its components' operation gives
template <typename X>
struct D3T {
  X x, y, z;
};
using D3 = D3T<Dual>;
template <typename A, typename B>
__device__ __forceinline__ auto operator+(D3T<A> a, D3T<B> b) -> D3T<decltype(a.x + b.x)> { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
template <typename A, typename B>
__device__ __forceinline__ auto operator-(D3T<A> a, D3T<B> b) -> D3T<decltype(a.x - b.x)> { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename A>
__device__ __forceinline__ auto operator*(double s, D3T<A> a) -> D3T<decltype(s * a.x)> { return {s * a.x, s * a.y, s * a.z}; }
template <typename A>
__device__ __forceinline__ D3 operator*(Dual s, D3T<A> a) { return {s * a.x, s * a.y, s * a.z}; }
template <typename A, typename B>
__device__ __forceinline__ auto dcross(D3T<A> a, D3T<B> b) -> D3T<decltype(a.y * b.z - a.z * b.y)> {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <typename C, typename X>
__device__ __forceinline__ auto dmatvec(const C (&A)[9], D3T<X> x) -> D3T<decltype(A[0] * x.x + A[1] * x.y)> {
  return {A[0] * x.x + A[1] * x.y + A[2] * x.z, A[3] * x.x + A[4] * x.y + A[5] * x.z, A[6] * x.x + A[7] * x.y + A[8] * x.z};
}
template <typename X>
struct DMatT {
  X m[9];
};
template <typename A, typename B>
__device__ __forceinline__ auto rot(const DMatT<A>& R, D3T<B> x) -> D3T<decltype(R.m[0] * x.x + R.m[1] * x.y)> {
  return {R.m[0] * x.x + R.m[1] * x.y + R.m[2] * x.z, R.m[3] * x.x + R.m[4] * x.y + R.m[5] * x.z,
          R.m[6] * x.x + R.m[7] * x.y + R.m[8] * x.z};
}
template <typename A, typename B>
__device__ __forceinline__ auto rot_t(const DMatT<A>& R, D3T<B> x) -> D3T<decltype(R.m[0] * x.x + R.m[3] * x.y)> {
  return {R.m[0] * x.x + R.m[3] * x.y + R.m[6] * x.z, R.m[1] * x.x + R.m[4] * x.y + R.m[7] * x.z,
          R.m[2] * x.x + R.m[5] * x.y + R.m[8] * x.z};
}

// the point map: in[47] = [y(19), yh(19), zh(6), tf(3)], out[25] = [y_s(19), z(6)].  Two things are types here:
//   X   what an input is - a dual number (the tangent runs along an input, or along inputs and constants) or a plain
//       double (the tangent runs along the constants alone: no operation among inputs carries one)
//   PC  where the constants come from - RodConst<double> (plain constants) or a structure with the same member names whose
//       rhoA, Ksei, Kbti, Bse, Bbt, rhoJ, Kse_vstar, rhoAg, C are dual numbers (RodConstDual, kr_adj_impl.hpp: the tangent
//       runs along a material parameter); c0 is plain in both.
// out is dual in every combination served.
template <typename X, typename PC>
__device__ __forceinline__ void point_map_dual(const PC& P, const X (&in)[47], bool cut, Dual (&out)[25]) {
  const X a = in[3], b = in[4], c = in[5], e = in[6];
  const D3T<X> n{in[7], in[8], in[9]}, m{in[10], in[11], in[12]}, q{in[13], in[14], in[15]}, w{in[16], in[17], in[18]};
  const D3T<X> yh_q{in[19 + 13], in[19 + 14], in[19 + 15]}, yh_w{in[19 + 16], in[19 + 17], in[19 + 18]};
  const D3T<X> vh{in[38], in[39], in[40]}, uh{in[41], in[42], in[43]};
  const D3T<X> tf{in[44], in[45], in[46]};
  // R = I + (2 / h.h) quad(h); cut: the entries of quad(h) are leaves
  const X aq = cut ? detach(a) : a, bq = cut ? detach(b) : b, cq = cut ? detach(c) : c, eq = cut ? detach(e) : e;
  const X s = 2.0 * dual_rcp(a * a + b * b + c * c + e * e);
  DMatT<X> R;
  R.m[0] = s * (-(cq * cq) - eq * eq) + 1.0; R.m[1] = s * (bq * cq - eq * aq);        R.m[2] = s * (bq * eq + cq * aq);
  R.m[3] = s * (bq * cq + eq * aq);          R.m[4] = s * (-(bq * bq) - eq * eq) + 1.0; R.m[5] = s * (cq * eq - bq * aq);
  R.m[6] = s * (bq * eq - cq * aq);          R.m[7] = s * (cq * eq + bq * aq);        R.m[8] = s * (-(bq * bq) - cq * cq) + 1.0;
  const D3 ksv{dual_of(P.Kse_vstar[0]), dual_of(P.Kse_vstar[1]), dual_of(P.Kse_vstar[2])};
  const D3 v = dmatvec(P.Ksei, rot_t(R, n) + ksv - dmatvec(P.Bse, vh));
  const D3 u = dmatvec(P.Kbti, rot_t(R, m) - dmatvec(P.Bbt, uh));
  const D3T<X> qt = P.c0 * q + yh_q, wt = P.c0 * w + yh_w;
  const D3 vt = P.c0 * v + vh, ut = P.c0 * u + uh;
  const D3T<decltype(P.C[0] * q.x)> drag{P.C[0] * (q.x * dual_abs(q.x)), P.C[1] * (q.y * dual_abs(q.y)), P.C[2] * (q.z * dual_abs(q.z))};
  const D3 rag{dual_of(P.rhoAg[0]), dual_of(P.rhoAg[1]), dual_of(P.rhoAg[2])};
  const D3 load = rag - rot(R, drag) + tf;
  const D3 ps = rot(R, v);
  const D3 ns = P.rhoA * rot(R, dcross(w, q) + qt) - load;
  const D3 ms = rot(R, dcross(w, dmatvec(P.rhoJ, w)) + dmatvec(P.rhoJ, wt)) - dcross(ps, n);
  const D3 qs = vt - dcross(u, q) + dcross(w, v);
  const D3 ws = ut - dcross(u, w);
  // h_s = 0.5 Omega(u) h; cut: the entries of Omega(u) are leaves
  const Dual u0 = cut ? detach(u.x) : u.x, u1 = cut ? detach(u.y) : u.y, u2 = cut ? detach(u.z) : u.z;
  out[0] = ps.x; out[1] = ps.y; out[2] = ps.z;
  out[3] = 0.5 * (-(u0 * b) - u1 * c - u2 * e);
  out[4] = 0.5 * (u0 * a + u2 * c - u1 * e);
  out[5] = 0.5 * (u1 * a - u2 * b + u0 * e);
  out[6] = 0.5 * (u2 * a + u1 * b - u0 * c);
  out[7] = ns.x; out[8] = ns.y; out[9] = ns.z;
  out[10] = ms.x; out[11] = ms.y; out[12] = ms.z;
  out[13] = qs.x; out[14] = qs.y; out[15] = qs.z;
  out[16] = ws.x; out[17] = ws.y; out[18] = ws.z;
  out[19] = v.x; out[20] = v.y; out[21] = v.z;
  out[22] = u.x; out[23] = u.y; out[24] = u.z;
}

}  // namespace kr
