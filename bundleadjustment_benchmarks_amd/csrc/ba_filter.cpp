// ba_filter.cpp -- the host-only part of ba_solver_filter_observations (include/ba_mi355x.h): the per-point rule of
// ba_filter.hip.h with one lane and the full pair loop, on arrays the caller hands over, the defaults and the parameter check.  No GPU,
// no solver: a CPU test calls these directly.
#include "ba_internal.h"
#include "ba_filter.hip.h"

#include <cmath>
#include <vector>

namespace {
struct HostTrack {
    unsigned char *st;
    const double *rays; // [t][3]
    int status(int i) const { return (int)st[i]; }
    void set_status(int i, int s) { st[i] = (unsigned char)s; }
    void ray(int i, double d[3]) const { for (int k = 0; k < 3; k++) d[k] = rays[3 * (size_t)i + k]; }
};
struct HostRed {
    double sum(double v) const { return v; }
    double max(double v) const { return v; }
};
} // namespace

// the kernel's status numbers are the public enums'
static_assert(BA_FLT_K_KEPT == BA_OBS_KEPT && BA_FLT_K_WAS_OFF == BA_OBS_WAS_OFF && BA_FLT_K_BEHIND == BA_OBS_BEHIND &&
                  BA_FLT_K_NONFINITE == BA_OBS_NONFINITE && BA_FLT_K_REPROJ == BA_OBS_REPROJ && BA_FLT_K_POINT == BA_OBS_POINT &&
                  BA_FLT_K_PT_KEPT == BA_FPT_KEPT && BA_FLT_K_PT_SHORT == BA_FPT_SHORT && BA_FLT_K_PT_LOW_ANGLE == BA_FPT_LOW_ANGLE,
              "ba_filter.hip.h restates ba_obs_status and ba_filter_point_status");

int ba_filter_params_check(const ba_filter_params *p)
{
    if (!p) return BA_ERR_ARG;
    if (!std::isfinite(p->max_reproj_px) || p->max_reproj_px < 0) return BA_ERR_ARG;
    if (!std::isfinite(p->min_angle_deg) || p->min_angle_deg < 0 || !(p->min_angle_deg < 180)) return BA_ERR_ARG;
    if (p->min_track < 0) return BA_ERR_ARG;
    return BA_OK;
}

extern "C" {

void ba_filter_params_default(ba_filter_params *p)
{
    if (!p) return;
    p->max_reproj_px = 4.0;
    p->min_angle_deg = 1.5;
    p->min_track = 2;
    p->require_front = 1;
}

int ba_filter_track(int t, const double *cam15, const double *meas, const unsigned char *active, const double *X, const ba_filter_params *p,
                    unsigned char *obs_status, int *pt_status, double *err_px, double *angle_deg)
{
    ba_filter_params pp;
    if (p) pp = *p; else ba_filter_params_default(&pp);
    if (ba_filter_params_check(&pp) || t < 0 || (t > 0 && (!cam15 || !meas)) || !X) return BA_ERR_ARG;
    const double amin = pp.min_angle_deg * (M_PI / 180.0);
    const ba_flt_cfg cf{pp.max_reproj_px, amin, ba_flt_chord2_exit(amin), pp.min_track, pp.require_front != 0};
    const size_t n = (size_t)(t > 0 ? t : 1);
    std::vector<unsigned char> st(n, 0);
    std::vector<double> rays(3 * n, 0.0);
    for (int i = 0; i < t; i++) {
        double er = NAN;
        st[i] = BA_FLT_K_WAS_OFF;
        if (!active || active[i]) {
            ba_flt_obs o;
            for (int k = 0; k < 15; k++) o.c[k] = cam15[(size_t)15 * i + k];
            o.m0 = meas[2 * (size_t)i]; o.m1 = meas[2 * (size_t)i + 1];
            st[i] = (unsigned char)ba_flt_observation(o, X, cf, er, &rays[3 * (size_t)i]);
        }
        if (err_px) err_px[i] = er;
    }
    HostTrack tk{st.data(), rays.data()};
    int ps;
    double ang;
    ba_flt_point<1, false>(0, t, tk, HostRed{}, cf, ps, ang);
    for (int i = 0; obs_status && i < t; i++) obs_status[i] = st[i];
    if (pt_status) *pt_status = ps;
    if (angle_deg) *angle_deg = ang * (180.0 / M_PI);
    return BA_OK;
}

} // extern "C"
