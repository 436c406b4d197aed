// Device camera models shared by the tracker-side kernels (rot_ransac.hip, ransac5.hip, ransac3.hip, upright2p.hip, stereo_gate.hip,
// trail_index.hip, flow_predict.hip): tracker::Camera's pixelToRay / rayToPixel (src/tracker/camera.cpp:93-221 pinhole, :264-398 fisheye) and
// normalizePixel (:471-476) in double precision, in the oracle's operation order.
#pragma once

#include "hv_internal.hpp"

namespace hv {
namespace {

// ---- camera models (camera.cpp), double precision, the oracle's operation order ----
__device__ inline void pin_distort(const hv_camera_model &c, double &x, double &y, double *J)
{
    if (!c.distortion_enabled) { J[0] = 1; J[1] = 0; J[2] = 0; J[3] = 1; return; }
    const double *k = c.coeffs, X = x, Y = y, r2 = X * X + Y * Y;
    const double theta = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]));
    const double dth = k[0] + r2 * (k[1] * 2 + r2 * k[2] * 3);
    J[0] = theta + X * dth * 2 * X; J[1] = X * dth * 2 * Y;
    J[2] = Y * dth * 2 * X;         J[3] = theta + Y * dth * 2 * Y;
    x = X * theta; y = Y * theta;
}

__device__ inline double fish_distort(const hv_camera_model &c, double theta, double *der)
{
    if (!c.distortion_enabled) { if (der) *der = 1.0; return theta; }
    const double *k = c.coeffs, t = theta, t2 = t * t;
    if (der) *der = 1 + 3 * t2 * (k[0] + 5.0 / 3 * t2 * (k[1] + 7.0 / 5 * t2 * (k[2] + 9.0 / 7 * t2 * k[3])));
    return t * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
}

__device__ inline double fish_newton(const hv_camera_model &c, double r, double theta0)
{
    const double eps = 0.01 / ((c.fx + c.fy) * 0.5);
    double theta = theta0, d;
    for (int it = 0; it < 20; ++it) {
        const double dr = fish_distort(c, theta, &d) - r, dt = dr / d;
        theta -= dt;
        if (fabs(dt) < eps) return theta > 0.0 ? theta : 0.0;
    }
    return -1;
}

__device__ inline bool pixel_to_ray(const hv_camera_model &c, double px, double py, double *ray)   // false: pixelToRay failed (fisheye r > maxValidR)
{
    if (c.kind == 0) {                                                       // camera.cpp:169-180
        double x = (px - c.ppx) / c.fx, y = (py - c.ppy) / c.fy;
        if (c.distortion_enabled) {                                          // :108-123 Newton
            const double dx = x, dy = y;
            double nrm;
            int it = 0;
            do {
                double qx = x, qy = y, J[4];
                pin_distort(c, qx, qy, J);
                const double id = 1.0 / (J[0] * J[3] - J[1] * J[2]);
                const double ex = dx - qx, ey = dy - qy;
                const double sx = (J[3] * id) * ex + (-J[1] * id) * ey, sy = (-J[2] * id) * ex + (J[0] * id) * ey;
                x += sx; y += sy;
                nrm = sqrt(sx * sx + sy * sy);
            } while (nrm > 1e-5 && ++it < 100);
        }
        const double n = sqrt(x * x + y * y + 1.0);
        double r[3] = {x / n, y / n, 1.0 / n};
        if (c.rotation_enabled) {
            const double *R = c.rotation;
            const double t0 = R[0] * r[0] + R[1] * r[1] + R[2] * r[2], t1 = R[3] * r[0] + R[4] * r[1] + R[5] * r[2],
                         t2 = R[6] * r[0] + R[7] * r[1] + R[8] * r[2];
            r[0] = t0; r[1] = t1; r[2] = t2;
        }
        ray[0] = r[0]; ray[1] = r[1]; ray[2] = r[2];
        return true;
    }
    const double *Ki = c.kinv;                                               // :353-375
    const double u = Ki[0] * px + Ki[1] * py + Ki[2], v = Ki[3] * px + Ki[4] * py + Ki[5];
    const double r = sqrt(u * u + v * v), dxn = u / r, dyn = v / r;
    double theta = r;
    if (r > c.max_r) theta = c.max_theta;
    else if (c.distortion_enabled) {
        const int n = c.n_table;
        double f = r / c.max_r; if (!(f > 0.0)) f = 0.0;
        int i = (int)(f * (double)n); if (i > n - 1) i = n - 1;
        const double th = fish_newton(c, r, c.table[i]);
        theta = th < 0 ? r : th;
    }
    const double s = sin(theta);
    ray[0] = s * dxn; ray[1] = s * dyn; ray[2] = cos(theta);
    return r <= c.max_r;
}

__device__ inline bool ray_to_pixel(const hv_camera_model &c, const double *ray0, double *pix)
{
    if (c.kind == 0) {                                                       // camera.cpp:182-205
        double r[3] = {ray0[0], ray0[1], ray0[2]};
        if (c.rotation_enabled) {
            const double *R = c.rotation;
            const double t0 = R[0] * r[0] + R[3] * r[1] + R[6] * r[2], t1 = R[1] * r[0] + R[4] * r[1] + R[7] * r[2],
                         t2 = R[2] * r[0] + R[5] * r[1] + R[8] * r[2];
            r[0] = t0; r[1] = t1; r[2] = t2;
        }
        if (r[2] <= 0) return false;
        const double iz = 1.0 / r[2];
        double x = r[0] * iz, y = r[1] * iz, J[4];
        pin_distort(c, x, y, J);
        pix[0] = c.fx * x + 0.0 * y + c.ppx * (r[2] * iz);
        pix[1] = 0.0 * x + c.fy * y + c.ppy * (r[2] * iz);
        return true;
    }
    if (ray0[2] <= 0) return false;                                          // :377-398
    const double inv = 1.0 / sqrt(ray0[0] * ray0[0] + ray0[1] * ray0[1] + ray0[2] * ray0[2]);
    const double theta = acos(ray0[2] * inv);
    if (theta > c.max_theta) return false;
    const double r = fish_distort(c, theta, nullptr);
    const double n2 = ray0[0] * ray0[0] + ray0[1] * ray0[1];
    double dx = ray0[0], dy = ray0[1];
    if (n2 > 0) { const double n = sqrt(n2); dx /= n; dy /= n; }
    const double u = r * dx, v = r * dy;
    pix[0] = c.fx * u + 0.0 * v + c.ppx;
    pix[1] = 0.0 * u + c.fy * v + c.ppy;
    return true;
}

// Camera::normalizePixel (camera.cpp:471-476) of a binary32 corner, with the reference's test: `ray.z() <= 0` fails, so a NaN depth
// passes (trail_index.hip)
__device__ inline bool normalize_pixel(const hv_camera_model &c, float x, float y, double *out)
{
    double r[3];
    if (!pixel_to_ray(c, (double)x, (double)y, r) || r[2] <= 0) return false;
    out[0] = r[0] / r[2]; out[1] = r[1] / r[2];
    return true;
}
// The same with the test of the RANSAC restatements (tests/ransac5_restatement.py: normalize, ransac3_restatement.py:
// normalize_pixel): only `r[2] > 0` passes, so a NaN depth fails. The two differ on NaN alone and are not merged: the RANSAC kernels
// equal their restatements, which drop such a point, and the trail keeps the reference's comparison.
__device__ inline bool normalize_pixel_positive(const hv_camera_model &c, float x, float y, double *out)
{
    double r[3];
    if (!(pixel_to_ray(c, (double)x, (double)y, r) && r[2] > 0)) return false;
    out[0] = r[0] / r[2]; out[1] = r[1] / r[2];
    return true;
}

}  // namespace
}  // namespace hv
