// ba_triangulate.cpp -- the host-only part of ba_solver_triangulate_points (include/ba_mi355x.h): the per-point
// rule of ba_triangulate.hip.h with one lane, on arrays the caller hands over, and the defaults.  No GPU, no solver: a CPU test calls
// these directly.
#include "ba_internal.h"
#include "ba_triangulate.hip.h"

#include <cmath>
#include <vector>

namespace {
struct HostObs {
    const double *cam15, *meas, *w;
    const double *rays; // [t][3]
    void load(int i, ba_tri_obs &o) const
    {
        for (int k = 0; k < 15; k++) o.c[k] = cam15[(size_t)15 * i + k];
        o.m0 = meas[2 * (size_t)i]; o.m1 = meas[2 * (size_t)i + 1];
        o.w = w ? w[i] : 1.0;
    }
    void ray(int i, double d[3]) const { for (int k = 0; k < 3; k++) d[k] = rays[3 * (size_t)i + k]; }
    bool active(int) const { return true; } // (the caller passes the active observations)
};
struct HostRed {
    double sum(double v) const { return v; }
    double max(double v) const { return v; }
};
} // namespace

// the kernel's status numbers are the public enum's
static_assert(BA_TRI_K_REPLACED == BA_TRI_REPLACED && BA_TRI_K_FEW_VIEWS == BA_TRI_FEW_VIEWS && BA_TRI_K_LOW_ANGLE == BA_TRI_LOW_ANGLE &&
                  BA_TRI_K_DEGENERATE == BA_TRI_DEGENERATE && BA_TRI_K_BEHIND == BA_TRI_BEHIND && BA_TRI_K_REPROJ == BA_TRI_REPROJ &&
                  BA_TRI_K_NOT_BETTER == BA_TRI_NOT_BETTER && BA_TRI_K_FIXED == BA_TRI_FIXED,
              "ba_triangulate.hip.h restates ba_triangulate_status");

int ba_triangulate_params_check(const ba_triangulate_params *p)
{
    if (!p) return BA_ERR_ARG;
    if (!std::isfinite(p->min_angle_deg) || p->min_angle_deg < 0 || !(p->min_angle_deg < 180)) return BA_ERR_ARG;
    if (!std::isfinite(p->max_reproj_px) || p->max_reproj_px < 0 || p->refine_iters < 0) return BA_ERR_ARG;
    return BA_OK;
}

extern "C" {

void ba_triangulate_params_default(ba_triangulate_params *p)
{
    if (!p) return;
    p->min_angle_deg = 1.5;
    p->max_reproj_px = 0;
    p->refine_iters = 5;
    p->only_if_better = 1;
}

int ba_triangulate_point(int t, const double *cam15, const double *meas, const double *w, int loss_kind, double loss_scale,
                         const ba_triangulate_params *p, const double *x_old, double *x_new, int *status, double *cost_old, double *cost_new,
                         double *angle_deg)
{
    ba_triangulate_params pp;
    if (p) pp = *p; else ba_triangulate_params_default(&pp);
    if (ba_triangulate_params_check(&pp) || t < 0 || (t > 0 && (!cam15 || !meas)) || !x_old) return BA_ERR_ARG;
    if (loss_kind < BA_LOSS_REFERENCE || loss_kind > BA_LOSS_CAUCHY) return BA_ERR_ARG;
    if (loss_kind != BA_LOSS_TRIVIAL && (!(loss_scale > 0) || !std::isfinite(loss_scale))) return BA_ERR_ARG;
    for (int i = 0; w && i < t; i++)
        if (!(w[i] > 0) || !std::isfinite(w[i])) return BA_ERR_ARG;
    std::vector<double> rays((size_t)3 * (t > 0 ? t : 1), 0.0);
    const HostObs ob{cam15, meas, w, rays.data()};
    for (int i = 0; i < t; i++) {
        ba_tri_obs o;
        ob.load(i, o);
        (void)ba_tri_ray(o, &rays[(size_t)3 * i]);
    }
    const ba_tri_cfg cf{pp.min_angle_deg * (M_PI / 180.0), pp.max_reproj_px, pp.refine_iters, pp.only_if_better, loss_kind,
                        loss_kind == BA_LOSS_TRIVIAL ? 1.0 : loss_scale};
    ba_tri_out out;
    ba_tri_point<1>(0, t, ob, HostRed{}, cf, x_old, 0, out);
    if (x_new) for (int k = 0; k < 3; k++) x_new[k] = out.x[k];
    if (status) *status = out.status;
    if (cost_old) *cost_old = out.cost_old;
    if (cost_new) *cost_new = out.cost_new;
    if (angle_deg) *angle_deg = out.angle_rad * (180.0 / M_PI);
    return BA_OK;
}

} // extern "C"
