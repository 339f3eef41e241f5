// Second- and third-order forward duals in one variable (value and its first two or three derivatives), first-order
// forward dual in N variables (value and gradient) and the closed-form site fraction of one associating component,
// shared by gnx_pcsaft.hip (pure components) and gnx_pcsaft_mix.hpp (mixtures).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace {

// ---- second-order forward dual --------------------------------------------------------------------------------------
struct D2 {
  double v, d, dd;
};
__device__ __forceinline__ D2 operator+(D2 a, D2 b) { return {a.v + b.v, a.d + b.d, a.dd + b.dd}; }
__device__ __forceinline__ D2 operator-(D2 a, D2 b) { return {a.v - b.v, a.d - b.d, a.dd - b.dd}; }
__device__ __forceinline__ D2 operator-(D2 a) { return {-a.v, -a.d, -a.dd}; }
__device__ __forceinline__ D2 operator+(D2 a, double b) { return {a.v + b, a.d, a.dd}; }
__device__ __forceinline__ D2 operator+(double b, D2 a) { return {a.v + b, a.d, a.dd}; }
__device__ __forceinline__ D2 operator-(D2 a, double b) { return {a.v - b, a.d, a.dd}; }
__device__ __forceinline__ D2 operator-(double b, D2 a) { return {b - a.v, -a.d, -a.dd}; }
__device__ __forceinline__ D2 operator*(D2 a, double b) { return {a.v * b, a.d * b, a.dd * b}; }
__device__ __forceinline__ D2 operator*(double b, D2 a) { return {a.v * b, a.d * b, a.dd * b}; }
__device__ __forceinline__ D2 operator*(D2 a, D2 b) {
  return {a.v * b.v, a.d * b.v + a.v * b.d, a.dd * b.v + 2.0 * a.d * b.d + a.v * b.dd};
}
__device__ __forceinline__ D2 operator/(D2 a, D2 b) {
  const double q = a.v / b.v;
  const double qd = (a.d - q * b.d) / b.v;
  return {q, qd, (a.dd - 2.0 * qd * b.d - q * b.dd) / b.v};
}
__device__ __forceinline__ D2 operator/(D2 a, double b) { return {a.v / b, a.d / b, a.dd / b}; }
__device__ __forceinline__ D2 operator/(double a, D2 b) { return D2{a, 0.0, 0.0} / b; }
__device__ __forceinline__ D2 exp(D2 a) {
  const double e = ::exp(a.v);
  return {e, e * a.d, e * (a.dd + a.d * a.d)};
}
__device__ __forceinline__ D2 log(D2 a) { return {::log(a.v), a.d / a.v, a.dd / a.v - (a.d * a.d) / (a.v * a.v)}; }
__device__ __forceinline__ D2 sqrt(D2 a) {
  const double s = ::sqrt(a.v);
  return {s, a.d / (2.0 * s), a.dd / (2.0 * s) - (a.d * a.d) / (4.0 * s * a.v)};
}
__device__ __forceinline__ double value_of(D2 a) { return a.v; }
__device__ __forceinline__ double value_of(double a) { return a; }
__device__ __forceinline__ double exp(double a) { return ::exp(a); }
__device__ __forceinline__ double log(double a) { return ::log(a); }
__device__ __forceinline__ double sqrt(double a) { return ::sqrt(a); }
__device__ __forceinline__ double expm1(double a) { return ::expm1(a); }

// ---- third-order forward dual: (value, d, d2, d3) in one variable, the operator set of D2 ----------------------------
// p_rho and p_rhorho of the critical-point conditions need a''' (gnx_pcsaft.hip).  Products and quotients by Leibniz's
// rule, exp / log / sqrt from the derivatives of their defining relations (e' = e a', l' a = a', s s = a).
struct D3 {
  double v, d, dd, d3;
};
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return {a.v + b.v, a.d + b.d, a.dd + b.dd, a.d3 + b.d3}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return {a.v - b.v, a.d - b.d, a.dd - b.dd, a.d3 - b.d3}; }
__device__ __forceinline__ D3 operator-(D3 a) { return {-a.v, -a.d, -a.dd, -a.d3}; }
__device__ __forceinline__ D3 operator+(D3 a, double b) { return {a.v + b, a.d, a.dd, a.d3}; }
__device__ __forceinline__ D3 operator+(double b, D3 a) { return {a.v + b, a.d, a.dd, a.d3}; }
__device__ __forceinline__ D3 operator-(D3 a, double b) { return {a.v - b, a.d, a.dd, a.d3}; }
__device__ __forceinline__ D3 operator-(double b, D3 a) { return {b - a.v, -a.d, -a.dd, -a.d3}; }
__device__ __forceinline__ D3 operator*(D3 a, double b) { return {a.v * b, a.d * b, a.dd * b, a.d3 * b}; }
__device__ __forceinline__ D3 operator*(double b, D3 a) { return {a.v * b, a.d * b, a.dd * b, a.d3 * b}; }
__device__ __forceinline__ D3 operator*(D3 a, D3 b) {
  return {a.v * b.v, a.d * b.v + a.v * b.d, a.dd * b.v + 2.0 * a.d * b.d + a.v * b.dd,
          a.d3 * b.v + 3.0 * a.dd * b.d + 3.0 * a.d * b.dd + a.v * b.d3};
}
__device__ __forceinline__ D3 operator/(D3 a, D3 b) {
  const double q = a.v / b.v;
  const double qd = (a.d - q * b.d) / b.v;
  const double qdd = (a.dd - 2.0 * qd * b.d - q * b.dd) / b.v;
  return {q, qd, qdd, (a.d3 - 3.0 * qdd * b.d - 3.0 * qd * b.dd - q * b.d3) / b.v};
}
__device__ __forceinline__ D3 operator/(D3 a, double b) { return {a.v / b, a.d / b, a.dd / b, a.d3 / b}; }
__device__ __forceinline__ D3 operator/(double a, D3 b) { return D3{a, 0.0, 0.0, 0.0} / b; }
__device__ __forceinline__ D3 exp(D3 a) {
  const double e = ::exp(a.v);
  const double ed = e * a.d;
  const double edd = ed * a.d + e * a.dd;
  return {e, ed, edd, edd * a.d + 2.0 * ed * a.dd + e * a.d3};
}
__device__ __forceinline__ D3 log(D3 a) {
  const double ld = a.d / a.v;
  const double ldd = (a.dd - ld * a.d) / a.v;
  return {::log(a.v), ld, ldd, (a.d3 - 2.0 * ldd * a.d - ld * a.dd) / a.v};
}
__device__ __forceinline__ D3 sqrt(D3 a) {
  const double s = ::sqrt(a.v);
  const double sd = a.d / (2.0 * s);
  const double sdd = (a.dd - 2.0 * sd * sd) / (2.0 * s);
  return {s, sd, sdd, (a.d3 - 6.0 * sd * sdd) / (2.0 * s)};
}
__device__ __forceinline__ double value_of(D3 a) { return a.v; }

// ---- first-order forward "gradient" dual: a value and its partial derivatives in N independent variables -------------
// The operator set of D2.  A double converts to a constant (all partials zero), so code written for double or D2
// coefficients instantiates on it unchanged.
template <int N>
struct DG {
  double v, g[N];
  DG() = default;
  __device__ __forceinline__ DG(double c) : v(c) {
#pragma unroll
    for (int k = 0; k < N; ++k) g[k] = 0.0;
  }
  // the k-th independent variable at the value c
  __device__ __forceinline__ static DG seed(double c, int k) {
    DG r(c);
    r.g[k] = 1.0;
    return r;
  }
};
// f(a) with f'(a) = fp, and f(a, b) with the partials fa, fb
template <int N>
__device__ __forceinline__ DG<N> dg_chain(double f, double fp, const DG<N>& a) {
  DG<N> r;
  r.v = f;
#pragma unroll
  for (int k = 0; k < N; ++k) r.g[k] = fp * a.g[k];
  return r;
}
template <int N>
__device__ __forceinline__ DG<N> dg_chain(double f, double fa, const DG<N>& a, double fb, const DG<N>& b) {
  DG<N> r;
  r.v = f;
#pragma unroll
  for (int k = 0; k < N; ++k) r.g[k] = fa * a.g[k] + fb * b.g[k];
  return r;
}
template <int N>
__device__ __forceinline__ DG<N> operator+(const DG<N>& a, const DG<N>& b) { return dg_chain(a.v + b.v, 1.0, a, 1.0, b); }
template <int N>
__device__ __forceinline__ DG<N> operator-(const DG<N>& a, const DG<N>& b) { return dg_chain(a.v - b.v, 1.0, a, -1.0, b); }
template <int N>
__device__ __forceinline__ DG<N> operator-(const DG<N>& a) { return dg_chain(-a.v, -1.0, a); }
template <int N>
__device__ __forceinline__ DG<N> operator+(const DG<N>& a, double b) { return dg_chain(a.v + b, 1.0, a); }
template <int N>
__device__ __forceinline__ DG<N> operator+(double b, const DG<N>& a) { return dg_chain(a.v + b, 1.0, a); }
template <int N>
__device__ __forceinline__ DG<N> operator-(const DG<N>& a, double b) { return dg_chain(a.v - b, 1.0, a); }
template <int N>
__device__ __forceinline__ DG<N> operator-(double b, const DG<N>& a) { return dg_chain(b - a.v, -1.0, a); }
template <int N>
__device__ __forceinline__ DG<N> operator*(const DG<N>& a, double b) { return dg_chain(a.v * b, b, a); }
template <int N>
__device__ __forceinline__ DG<N> operator*(double b, const DG<N>& a) { return dg_chain(a.v * b, b, a); }
template <int N>
__device__ __forceinline__ DG<N> operator*(const DG<N>& a, const DG<N>& b) { return dg_chain(a.v * b.v, b.v, a, a.v, b); }
template <int N>
__device__ __forceinline__ DG<N>& operator+=(DG<N>& a, const DG<N>& b) { return a = a + b; }
template <int N>
__device__ __forceinline__ DG<N>& operator*=(DG<N>& a, const DG<N>& b) { return a = a * b; }
template <int N>
__device__ __forceinline__ DG<N>& operator*=(DG<N>& a, double b) { return a = a * b; }
template <int N>
__device__ __forceinline__ DG<N> operator/(const DG<N>& a, const DG<N>& b) {
  const double q = a.v / b.v;
  return dg_chain(q, 1.0 / b.v, a, -q / b.v, b);
}
template <int N>
__device__ __forceinline__ DG<N> operator/(const DG<N>& a, double b) { return dg_chain(a.v / b, 1.0 / b, a); }
template <int N>
__device__ __forceinline__ DG<N> operator/(double a, const DG<N>& b) {
  const double q = a / b.v;
  return dg_chain(q, -q / b.v, b);
}
template <int N>
__device__ __forceinline__ DG<N> exp(const DG<N>& a) {
  const double e = ::exp(a.v);
  return dg_chain(e, e, a);
}
template <int N>
__device__ __forceinline__ DG<N> expm1(const DG<N>& a) { return dg_chain(::expm1(a.v), ::exp(a.v), a); }
template <int N>
__device__ __forceinline__ DG<N> log(const DG<N>& a) { return dg_chain(::log(a.v), 1.0 / a.v, a); }
template <int N>
__device__ __forceinline__ DG<N> sqrt(const DG<N>& a) {
  const double s = ::sqrt(a.v);
  return dg_chain(s, 0.5 / s, a);
}
template <int N>
__device__ __forceinline__ double value_of(const DG<N>& a) { return a.v; }
// a coefficient that multiplies nothing in: its value and, on a dual, every partial is zero
__device__ __forceinline__ bool is_zero(double a) { return a == 0.0; }
template <int N>
__device__ __forceinline__ bool is_zero(const DG<N>& a) {
  bool z = a.v == 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) z = z && a.g[k] == 0.0;
  return z;
}

// positive root of q X^2 + u X - 1 = 0 (q > 0), the mass-action law of one site type: X_A with u = 1 + (nb - na) x,
// q = na x.  Written so that neither branch cancels: 2 / (u + sqrt(u^2 + 4q)) for u >= 0, (sqrt(u^2 + 4q) - u) / 2q
// for u < 0.
template <typename R>
__device__ __forceinline__ R site_fraction(R u, R q) {
  const R s = sqrt(u * u + 4.0 * q);
  if (value_of(u) >= 0.0) return 2.0 / (u + s);
  return (s - u) / (2.0 * q);
}

}  // namespace
