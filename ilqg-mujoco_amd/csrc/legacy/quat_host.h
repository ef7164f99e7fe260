// Host restatement of the quaternion step that the device physics
// (csrc/device/dphys.h: det_sin / det_cos, normalize3, normalize4,
// axis_angle2quat, quat_mul, quat_integrate) and the test oracle share: the
// fdlibm/musl sin and cos kernels with Cody-Waite pi/2 reduction, the same
// constants and the same operation order, so that the legacy boundary's host
// side perturbs a quaternion to the very doubles the FD kernels do.  Built with
// -ffp-contract=off like every other unit of the arithmetic contract.
#pragma once

#include <cmath>

namespace ilqg_legacy {
namespace hostq {

constexpr double MINVAL = 1e-15;  // mjMINVAL

inline double k_sin(double x, double y, int iy) {
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
               S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
               S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  double z = x * x, w = z * z;
  double r = S2 + z * (S3 + z * S4) + z * w * (S5 + z * S6);
  double v = z * x;
  if (iy == 0) return x + v * (S1 + z * r);
  return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
inline double k_cos(double x, double y) {
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
               C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
               C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  double z = x * x, w = z * z;
  double r = z * (C1 + z * (C2 + z * C3)) + w * w * (C4 + z * (C5 + z * C6));
  double hz = 0.5 * z;
  w = 1.0 - hz;
  return w + (((1.0 - w) - hz) + (z * r - x * y));
}
inline int rem_pio2(double x, double* y0, double* y1) {
  const double INVPIO2 = 6.36619772367581382433e-01, PIO2_1 = 1.57079632673412561417e+00,
               PIO2_1T = 6.07710050650619224932e-11;
  double fn = std::floor(x * INVPIO2 + 0.5);
  double r = x - fn * PIO2_1;
  double w = fn * PIO2_1T;
  *y0 = r - w;
  *y1 = (r - *y0) - w;
  return (int)fn;
}
inline double det_sin(double x) {
  const double PIO4 = 7.85398163397448278999e-01;
  double y0, y1;
  if (std::fabs(x) < PIO4) return x == 0 ? x : k_sin(x, 0.0, 0);
  int n = rem_pio2(x, &y0, &y1);
  switch (n & 3) {
    case 0: return k_sin(y0, y1, 1);
    case 1: return k_cos(y0, y1);
    case 2: return -k_sin(y0, y1, 1);
    default: return -k_cos(y0, y1);
  }
}
inline double det_cos(double x) {
  const double PIO4 = 7.85398163397448278999e-01;
  double y0, y1;
  if (std::fabs(x) < PIO4) return k_cos(x, 0.0);
  int n = rem_pio2(x, &y0, &y1);
  switch (n & 3) {
    case 0: return k_cos(y0, y1);
    case 1: return -k_sin(y0, y1, 1);
    case 2: return -k_cos(y0, y1);
    default: return k_sin(y0, y1, 1);
  }
}

inline double normalize3(double* v) {
  double norm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (norm < MINVAL) {
    v[0] = 1; v[1] = 0; v[2] = 0;
  } else {
    double inv = 1 / norm;
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
  }
  return norm;
}
// a quaternion within MINVAL of unit length is left as it is
inline void normalize4(double* q) {
  double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (norm < MINVAL) {
    q[0] = 1; q[1] = 0; q[2] = 0; q[3] = 0;
  } else if (std::fabs(norm - 1) > MINVAL) {
    double inv = 1 / norm;
    q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv;
  }
}
inline void axis_angle2quat(double* r, const double* axis, double angle) {
  if (angle == 0) {
    r[0] = 1; r[1] = 0; r[2] = 0; r[3] = 0;
  } else {
    double s = det_sin(angle * 0.5);
    r[0] = det_cos(angle * 0.5);
    r[1] = axis[0] * s; r[2] = axis[1] * s; r[3] = axis[2] * s;
  }
}
inline void quat_mul(double* r, const double* a, const double* b) {
  double t0 = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  double t1 = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  double t2 = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  double t3 = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = t0; r[1] = t1; r[2] = t2; r[3] = t3;
}
inline void quat_integrate(double* quat, const double* vel, double scale) {
  double tmp[3] = {vel[0], vel[1], vel[2]}, qrot[4];
  double angle = scale * normalize3(tmp);
  axis_angle2quat(qrot, tmp, angle);
  normalize4(quat);
  quat_mul(quat, quat, qrot);
}

}  // namespace hostq
}  // namespace ilqg_legacy
