// The stereo triangulation of the two stereo track filters (ransac3.hip, upright2p.hip): one statement, in the operation order of
// tests/ransac3_restatement.py (triangulate_stereo_idp).
//
// No include guard and no namespace of its own, like hv_geometry.hpp, and included behind it (cross3, dot3): a translation unit
// includes it once, inside its anonymous namespace.

// triangulateStereoFeatureIdp (triangulation.cpp:711-764) and world_point = (idp.x, idp.y, 1) / idp.z (ransac_pipeline.cpp:244,
// stereo_upright_2p.cpp:142)
__device__ bool triangulate_world(const double *T, double fu, double fv, double su, double sv, double *X)
{
    const double f0[3] = {su, sv, 1.0}, f1[3] = {fu, fv, 1.0};
    const double n0 = sqrt(dot3(f0, f0)), n1 = sqrt(dot3(f1, f1));
    const double f0h[3] = {f0[0] / n0, f0[1] / n0, f0[2] / n0}, f1h[3] = {f1[0] / n1, f1[1] / n1, f1[2] / n1};
    const double t[3] = {T[3], T[7], T[11]};
    double Rf[3], a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) Rf[i] = (T[4 * i] * f0h[0] + T[4 * i + 1] * f0h[1]) + T[4 * i + 2] * f0h[2];
    double p[3], q[3], r[3];
    cross3(Rf, f1h, p); cross3(Rf, t, q); cross3(f1h, t, r);
    const double pn = sqrt(dot3(p, p)), qn = sqrt(dot3(q, q)), rn = sqrt(dot3(r, r));
    const double l0 = rn / pn, l1 = qn / pn, w = qn / (qn + rn);
    double pf[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pf[i] = w * (t[i] + l0 * (Rf[i] + f1h[i]));
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = ((l0 * T[4 * i]) * f0h[0] + (l0 * T[4 * i + 1]) * f0h[1]) + (l0 * T[4 * i + 2]) * f0h[2];
    const double b[3] = {l1 * f1h[0], l1 * f1h[1], l1 * f1h[2]};
    double v0[3], v1[3], v2[3], v3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v0[i] = (t[i] + a[i]) - b[i]; v1[i] = (t[i] + a[i]) + b[i]; v2[i] = (t[i] - a[i]) - b[i]; v3[i] = (t[i] - a[i]) + b[i];
    }
    const double c0 = dot3(v0, v0), c1 = dot3(v1, v1), c2 = dot3(v2, v2), c3 = dot3(v3, v3);
    double mn = c2 < c1 ? c2 : c1;
    mn = c3 < mn ? c3 : mn;
    if (c0 > mn) return false;
    const double i0 = pf[0] / pf[2], i1 = pf[1] / pf[2], i2 = 1.0 / pf[2];
    X[0] = i0 / i2; X[1] = i1 / i2; X[2] = 1.0 / i2;
    return true;
}
