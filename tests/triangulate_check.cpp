// The host rule of ba_triangulate_point (csrc/ba_triangulate.cpp, csrc/ba_triangulate.hip.h) in a stand-alone program, built by
// tests/test_triangulate_cpu.py with the host compiler and -fsanitize=address,undefined: designed tracks whose answer is known by
// construction, and inputs chosen to walk every early exit of the rule (no observation, one, values that are not finite, a distortion
// without an inverse, parallel rays, refused arguments) with the sanitizers watching every index and operation.
#include "../include/ba_mi355x.h"

#include <cmath>
#include <cstdio>
#include <vector>

static int cases = 0, failures = 0;
static void check(bool ok, const char *what)
{
    cases++;
    if (!ok) { failures++; printf("FAILED: %s\n", what); }
}

// t cameras on an arc around X, each looking at X down its -z axis: 15 scalars per camera (R row-major, T, f, k1, k2)
static std::vector<double> arc(int t, const double X[3], double spread, double k1, double k2)
{
    std::vector<double> c((size_t)15 * (t > 0 ? t : 1), 0.0);
    for (int i = 0; i < t; i++) {
        const double a = spread * ((t > 1 ? (double)i / (t - 1) : 0.5) - 0.5), r = 6.0 + 0.5 * std::sin(3.0 * i);
        const double C[3] = {X[0] + r * std::sin(a), X[1] + 0.2 * std::cos(5.0 * i), X[2] + r * std::cos(a)};
        double z[3] = {C[0] - X[0], C[1] - X[1], C[2] - X[2]};
        const double nz = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
        for (double &v : z) v /= nz;
        double x[3] = {z[2], 0.0, -z[0]}; // (0, 1, 0) x z
        const double nx = std::sqrt(x[0] * x[0] + x[2] * x[2]);
        for (double &v : x) v /= nx;
        const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
        double *o = &c[(size_t)15 * i];
        for (int k = 0; k < 3; k++) { o[k] = x[k]; o[3 + k] = y[k]; o[6 + k] = z[k]; }
        for (int r3 = 0; r3 < 3; r3++) o[9 + r3] = -(o[3 * r3] * C[0] + o[3 * r3 + 1] * C[1] + o[3 * r3 + 2] * C[2]);
        o[12] = 800.0; o[13] = k1; o[14] = k2;
    }
    return c;
}

static std::vector<double> project(int t, const std::vector<double> &c, const double X[3])
{
    std::vector<double> m((size_t)2 * (t > 0 ? t : 1), 0.0);
    for (int i = 0; i < t; i++) {
        const double *o = &c[(size_t)15 * i];
        double XX[3];
        for (int r = 0; r < 3; r++) XX[r] = o[3 * r] * X[0] + o[3 * r + 1] * X[1] + o[3 * r + 2] * X[2] + o[9 + r];
        const double u0 = XX[0] / XX[2], u1 = XX[1] / XX[2], r2 = u0 * u0 + u1 * u1, kr = 1 + o[13] * r2 + o[14] * r2 * r2;
        m[2 * (size_t)i] = o[12] * kr * u0; m[2 * (size_t)i + 1] = o[12] * kr * u1;
    }
    return m;
}

int main()
{
    const double X[3] = {0.4, -0.2, 1.5}, X0[3] = {0.45, -0.23, 1.54};
    ba_triangulate_params p;
    ba_triangulate_params_default(&p);
    check(p.min_angle_deg == 1.5 && p.max_reproj_px == 0 && p.refine_iters == 5 && p.only_if_better == 1, "defaults");
    const int sizes[] = {2, 3, 8, 9, 64, 65, 300, 1500};
    for (int t : sizes)
        for (int loss = BA_LOSS_REFERENCE; loss <= BA_LOSS_CAUCHY; loss++) {
            const std::vector<double> c = arc(t, X, 1.0, -0.05, 0.01), m = project(t, c, X), w((size_t)t, 1.5);
            double xn[3], c0 = -1, c1 = -1, ang = -1;
            int st = -1;
            const int rc = ba_triangulate_point(t, c.data(), m.data(), loss & 1 ? w.data() : nullptr, loss, 0.5, &p, X0, xn, &st, &c0, &c1, &ang);
            const double err = std::fabs(xn[0] - X[0]) + std::fabs(xn[1] - X[1]) + std::fabs(xn[2] - X[2]);
            check(rc == BA_OK && st == BA_TRI_REPLACED && err < 1e-11 && c1 < 1e-18 && c0 > c1 && ang > 20 && ang < 90, "noiseless track returns the true X");
        }
    { // no observation, one observation, NULL outputs
        int st = -1;
        double xn[3] = {0, 0, 0}, c0 = -1;
        check(ba_triangulate_point(0, nullptr, nullptr, nullptr, 0, 0.5, nullptr, X0, xn, &st, &c0, nullptr, nullptr) == BA_OK && st == BA_TRI_FEW_VIEWS &&
                  xn[0] == X0[0] && c0 == 0, "t = 0");
        const std::vector<double> c = arc(1, X, 1.0, 0, 0), m = project(1, c, X);
        check(ba_triangulate_point(1, c.data(), m.data(), nullptr, 0, 0.5, &p, X0, nullptr, &st, nullptr, nullptr, nullptr) == BA_OK && st == BA_TRI_FEW_VIEWS, "t = 1");
        check(ba_triangulate_point(1, c.data(), m.data(), nullptr, 0, 0.5, &p, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_OK, "all outputs NULL");
    }
    { // measurements that are not finite, f = 0, a distortion without an inverse: unusable observations, never a fault
        std::vector<double> c = arc(4, X, 1.0, 0, 0), m = project(4, c, X);
        int st = -1;
        double xn[3];
        m[0] = NAN;
        check(ba_triangulate_point(4, c.data(), m.data(), nullptr, 0, 0.5, &p, X0, xn, &st, nullptr, nullptr, nullptr) == BA_OK && st != BA_TRI_FEW_VIEWS, "NaN measurement: three usable left");
        m[2] = INFINITY; m[4] = NAN;
        check(ba_triangulate_point(4, c.data(), m.data(), nullptr, 0, 0.5, &p, X0, xn, &st, nullptr, nullptr, nullptr) == BA_OK && st == BA_TRI_FEW_VIEWS, "one usable left");
        m = project(4, c, X);
        c[12] = 0.0;
        c[15 + 13] = -0.3; m[2] = 2 * 800.0; m[3] = 0;
        double ang = 0;
        check(ba_triangulate_point(4, c.data(), m.data(), nullptr, 0, 0.5, &p, X0, xn, &st, nullptr, nullptr, &ang) == BA_OK && st == BA_TRI_REPLACED &&
                  std::fabs(xn[0] - X[0]) < 1e-11, "f = 0 and no inverse: two usable observations give the true X");
    }
    { // parallel rays: the same camera twice
        std::vector<double> c = arc(1, X, 1.0, 0, 0), m = project(1, c, X);
        c.insert(c.end(), c.begin(), c.begin() + 15); m.insert(m.end(), m.begin(), m.begin() + 2);
        int st = -1;
        check(ba_triangulate_point(2, c.data(), m.data(), nullptr, 0, 0.5, &p, X0, nullptr, &st, nullptr, nullptr, nullptr) == BA_OK && st == BA_TRI_LOW_ANGLE, "parallel rays: LOW_ANGLE");
        ba_triangulate_params q = p;
        q.min_angle_deg = 0;
        check(ba_triangulate_point(2, c.data(), m.data(), nullptr, 0, 0.5, &q, X0, nullptr, &st, nullptr, nullptr, nullptr) == BA_OK && st == BA_TRI_DEGENERATE, "parallel rays without an angle test: DEGENERATE");
    }
    { // refusals
        const std::vector<double> c = arc(3, X, 1.0, 0, 0), m = project(3, c, X);
        const double wbad[3] = {1, 0, 1};
        ba_triangulate_params q = p;
        q.min_angle_deg = 180;
        check(ba_triangulate_point(3, c.data(), m.data(), nullptr, 0, 0.5, &q, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "angle 180");
        q = p; q.refine_iters = -1;
        check(ba_triangulate_point(3, c.data(), m.data(), nullptr, 0, 0.5, &q, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "refine_iters < 0");
        q = p; q.max_reproj_px = NAN;
        check(ba_triangulate_point(3, c.data(), m.data(), nullptr, 0, 0.5, &q, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "NaN bound");
        check(ba_triangulate_point(-1, c.data(), m.data(), nullptr, 0, 0.5, &p, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "t < 0");
        check(ba_triangulate_point(3, nullptr, m.data(), nullptr, 0, 0.5, &p, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "no cameras");
        check(ba_triangulate_point(3, c.data(), m.data(), nullptr, 0, 0.5, &p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "no x_old");
        check(ba_triangulate_point(3, c.data(), m.data(), wbad, 0, 0.5, &p, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "zero weight");
        check(ba_triangulate_point(3, c.data(), m.data(), nullptr, 9, 0.5, &p, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "unknown loss");
        check(ba_triangulate_point(3, c.data(), m.data(), nullptr, BA_LOSS_HUBER, 0.0, &p, X0, nullptr, nullptr, nullptr, nullptr, nullptr) == BA_ERR_ARG, "scale 0");
    }
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
