// Pose fitting, the minimal solver: one real root of a cubic and P3P (up to four poses from
// three bearings and three world points). Included after fit_work.h (dot3, cross3, sym_*).
#pragma once

namespace epos {
namespace {

__device__ __forceinline__ double cubic_eval(double x, double b, double c, double d) {
  return ((x + b) * x + c) * x + d;
}

// One real root of x^3 + b x^2 + c x + d: Newton started beyond the outer
// turning point (monotone convergence).
__device__ double cubic_root(double b, double c, double d) {
  double x;
  const double disc = b * b - 3.0 * c;
  if (disc > 0.0) {
    const double v = sqrt(disc);
    const double t1 = (-b - v) / 3.0;
    const double f1 = cubic_eval(t1, b, c, d);
    if (f1 > 0.0) {
      double step = v / 3.0 + 1e-3;
      x = t1 - step;
      for (int i = 0; i < 200 && cubic_eval(x, b, c, d) > 0.0; ++i) { step *= 2.0; x = t1 - step; }
    } else {
      const double t2 = (-b + v) / 3.0;
      double step = v / 3.0 + 1e-3;
      x = t2 + step;
      for (int i = 0; i < 200 && cubic_eval(x, b, c, d) < 0.0; ++i) { step *= 2.0; x = t2 + step; }
    }
  } else {
    const double t0 = -b / 3.0;
    const double f0 = cubic_eval(t0, b, c, d);
    double step = 1.0 + fabs(t0);
    x = t0;
    if (f0 > 0.0) {
      x = t0 - step;
      for (int i = 0; i < 200 && cubic_eval(x, b, c, d) > 0.0; ++i) { step *= 2.0; x = t0 - step; }
    } else if (f0 < 0.0) {
      x = t0 + step;
      for (int i = 0; i < 200 && cubic_eval(x, b, c, d) < 0.0; ++i) { step *= 2.0; x = t0 + step; }
    }
  }
  for (int i = 0; i < 60; ++i) {
    const double f = cubic_eval(x, b, c, d);
    const double fp = (3.0 * x + 2.0 * b) * x + c;
    if (fp == 0.0) break;
    const double dx = f / fp;
    x -= dx;
    if (fabs(dx) <= 1e-15 * fabs(x)) break;
  }
  return x;
}

// ------------------------------------------------------------------ P3P --
// f[9]: three unit bearings (row major), X[9]: three world points. Writes up to
// 4 poses (R row-major 9 + t 3) to pose[k*12]; returns their number.
__device__ int p3p(const double* f, const double* X, double* pose) {
  const double c12 = dot3(f, f + 3), c13 = dot3(f, f + 6), c23 = dot3(f + 3, f + 6);
  double d12[3], d13[3], d23[3];
  for (int i = 0; i < 3; ++i) {
    d12[i] = X[i] - X[3 + i];
    d13[i] = X[i] - X[6 + i];
    d23[i] = X[3 + i] - X[6 + i];
  }
  const double a12 = dot3(d12, d12), a13 = dot3(d13, d13), a23 = dot3(d23, d23);
  double nx[3];
  cross3(d12, d13, nx);
  const double detx = dot3(nx, nx);
  if (!(detx > 1e-18 * (a12 * a13 + 1e-300))) return 0;
  double r0[3], r1[3];
  cross3(d13, nx, r0);
  cross3(nx, d12, r1);
  double Xinv[9];
  for (int i = 0; i < 3; ++i) {
    Xinv[i] = r0[i] / detx;
    Xinv[3 + i] = r1[i] / detx;
    Xinv[6 + i] = nx[i] / detx;
  }
  const double M12[6] = {1, -c12, 0, 1, 0, 0};
  const double M13[6] = {1, 0, -c13, 0, 0, 1};
  const double M23[6] = {0, 0, 0, 1, -c23, 1};
  double D1[6], D2[6];
  for (int i = 0; i < 6; ++i) {
    D1[i] = a23 * M12[i] - a12 * M23[i];
    D2[i] = a23 * M13[i] - a13 * M23[i];
  }
  double A1[6], A2[6];
  sym_adj(D1, A1);
  sym_adj(D2, A2);
  const double k0 = sym_det(D1, A1), k3 = sym_det(D2, A2);
  const double k1 = sym_inner(A1, D2), k2 = sym_inner(A2, D1);
  double D0[6], E[6];
  if (fabs(k3) >= fabs(k0)) {
    if (k3 == 0.0) return 0;
    const double g = cubic_root(k2 / k3, k1 / k3, k0 / k3);
    const bool use2 = fabs(g) <= 1.0;
    for (int i = 0; i < 6; ++i) { D0[i] = D1[i] + g * D2[i]; E[i] = use2 ? D2[i] : D1[i]; }
  } else {
    const double g = cubic_root(k1 / k0, k2 / k0, k3 / k0);
    const bool use1 = fabs(g) <= 1.0;
    for (int i = 0; i < 6; ++i) { D0[i] = g * D1[i] + D2[i]; E[i] = use1 ? D1[i] : D2[i]; }
  }
  double B[6];
  sym_adj(D0, B);
  int bi = 0;
  double bmax = -B[0];
  if (-B[3] > bmax) { bmax = -B[3]; bi = 1; }
  if (-B[5] > bmax) { bmax = -B[5]; bi = 2; }
  if (!(bmax > 0.0)) return 0;
  const double sq = sqrt(bmax);
  double pt[3];
  for (int i = 0; i < 3; ++i) pt[i] = -sym_at(B, i, bi) / sq;
  double N[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) N[i * 3 + j] = sym_at(D0, i, j);
  N[1] -= pt[2]; N[2] += pt[1];
  N[3] += pt[2]; N[5] -= pt[0];
  N[6] -= pt[1]; N[7] += pt[0];
  int ri = 0, ci = 0;
  double rbest = -1.0, cbest = -1.0;
  for (int i = 0; i < 3; ++i) {
    const double rn = N[i * 3] * N[i * 3] + N[i * 3 + 1] * N[i * 3 + 1] + N[i * 3 + 2] * N[i * 3 + 2];
    const double cn = N[i] * N[i] + N[3 + i] * N[3 + i] + N[6 + i] * N[6 + i];
    if (rn > rbest) { rbest = rn; ri = i; }
    if (cn > cbest) { cbest = cn; ci = i; }
  }
  double planes[6];
  for (int j = 0; j < 3; ++j) { planes[j] = N[ri * 3 + j]; planes[3 + j] = N[j * 3 + ci]; }

  int nsol = 0;
  for (int pl = 0; pl < 2; ++pl) {
    const double* n = planes + 3 * pl;
    int k = 0;
    if (fabs(n[1]) > fabs(n[k])) k = 1;
    if (fabs(n[2]) > fabs(n[k])) k = 2;
    if (n[k] == 0.0) continue;
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const double ua = -n[a] / n[k], ub = -n[b] / n[k];
    const double Eaa = sym_at(E, a, a), Ebb = sym_at(E, b, b), Ekk = sym_at(E, k, k);
    const double Eab = sym_at(E, a, b), Eak = sym_at(E, a, k), Ebk = sym_at(E, b, k);
    const double q00 = Eaa + 2.0 * ua * Eak + ua * ua * Ekk;
    const double q11 = Ebb + 2.0 * ub * Ebk + ub * ub * Ekk;
    const double q01 = Eab + ub * Eak + ua * Ebk + ua * ub * Ekk;
    const double disc = q01 * q01 - q00 * q11;
    if (!(disc >= 0.0)) continue;
    const double sd = sqrt(disc);
    for (int sg = 0; sg < 2; ++sg) {
      double la, lb;
      const double num = sg == 0 ? (-q01 + sd) : (-q01 - sd);
      if (fabs(q00) >= fabs(q11)) {
        if (q00 == 0.0) continue;
        la = num / q00; lb = 1.0;
      } else {
        la = 1.0; lb = num / q11;
      }
      double lam[3];
      const double lk = ua * la + ub * lb;
      lam[0] = a == 0 ? la : (b == 0 ? lb : lk);
      lam[1] = a == 1 ? la : (b == 1 ? lb : lk);
      lam[2] = a == 2 ? la : (b == 2 ? lb : lk);
      const double qs = sym_quad(M12, lam) + sym_quad(M13, lam) + sym_quad(M23, lam);
      if (!(qs > 0.0)) continue;
      double sc = sqrt((a12 + a13 + a23) / qs);
      if (lam[0] < 0.0) sc = -sc;
      lam[0] *= sc; lam[1] *= sc; lam[2] *= sc;
      if (!(lam[0] > 0.0 && lam[1] > 0.0 && lam[2] > 0.0)) continue;
      double Y[9];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Y[i * 3 + j] = lam[i] * f[i * 3 + j];
      double e12[3], e13[3], ny[3];
      for (int j = 0; j < 3; ++j) { e12[j] = Y[j] - Y[3 + j]; e13[j] = Y[j] - Y[6 + j]; }
      cross3(e12, e13, ny);
      double* R = pose + nsol * 12;
      double* t = R + 9;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          R[i * 3 + j] = e12[i] * Xinv[j] + e13[i] * Xinv[3 + j] + ny[i] * Xinv[6 + j];
      for (int i = 0; i < 3; ++i)
        t[i] = Y[i] - (R[i * 3] * X[0] + R[i * 3 + 1] * X[1] + R[i * 3 + 2] * X[2]);
      ++nsol;
    }
  }
  return nsol;
}

}  // namespace
}  // namespace epos
