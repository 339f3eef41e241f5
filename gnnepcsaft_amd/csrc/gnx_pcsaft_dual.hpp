// Second-order forward dual in one variable (value, first and second derivative) and the closed-form site fraction of
// one associating component, shared by gnx_pcsaft.hip (pure components) and gnx_pcsaft_mix.hip (mixtures).
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
