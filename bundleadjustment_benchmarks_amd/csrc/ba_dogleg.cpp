// ba_dogleg.cpp -- the host-only part of Powell's dogleg (include/ba_mi355x.h): the step's coefficients and its
// predicted decrease from six scalars, and the driver's defaults.  No GPU, no solver: a CPU test calls these directly.
#include "../../include/ba_mi355x.h"

#include <cmath>

extern "C" {

int ba_dogleg_coefficients(double g2, double q, double gn2, double g_dot_gn, double mu, double radius, double *a_out, double *c_out,
                           int *branch_out, double *pred_out)
{
    const double d = g_dot_gn;
    if (!std::isfinite(g2) || !std::isfinite(q) || !std::isfinite(gn2) || !std::isfinite(d) || g2 < 0 || q < 0 || gn2 < 0 || d < 0) return BA_ERR_ARG;
    if (!(mu > 0) || !std::isfinite(mu) || !(radius > 0)) return BA_ERR_ARG; // (radius: NaN fails the comparison; inf is legal)
    if (g2 > 0 && !(q > 0)) return BA_ERR_ARG;
    double a = 0, c = 0, pred = 0;
    int branch = 0;
    if (g2 > 0) {
        const double alpha = g2 / q, ng = std::sqrt(g2);
        if (std::sqrt(gn2) <= radius) { a = 0; c = 1; branch = 0; }
        else if (alpha * ng >= radius) { a = radius / ng; c = 0; branch = 1; }
        else {
            // |dx_sd + beta (dx_gn - dx_sd)| = radius:  A beta^2 + 2 B beta + C = 0, the root in (0, 1] by the form that does not cancel
            const double A = gn2 - 2 * alpha * d + alpha * alpha * g2, B = alpha * d - alpha * alpha * g2, C = alpha * alpha * g2 - radius * radius;
            double disc = B * B - A * C;
            if (disc < 0) disc = 0;
            double beta = B <= 0 ? (-B + std::sqrt(disc)) / A : -C / (B + std::sqrt(disc));
            if (!(beta > 0)) beta = 0; // (A > 0 and C < 0 here in exact arithmetic; rounding at the edges only)
            if (beta > 1) beta = 1;
            a = alpha * (1 - beta); c = beta; branch = 2;
        }
        // 2 g'dx - dx'H dx with H dx_gn = g - mu dx_gn
        pred = 2 * (a * g2 + c * d) - (a * a * q + 2 * a * c * (g2 - mu * d) + c * c * (d - mu * gn2));
    }
    if (a_out) *a_out = a;
    if (c_out) *c_out = c;
    if (branch_out) *branch_out = branch;
    if (pred_out) *pred_out = pred;
    return BA_OK;
}

void ba_dogleg_params_default(ba_dogleg_params *p)
{
    if (!p) return;
    ba_lm_params lm;
    ba_lm_params_default(&lm);
    p->radius_init = 0;
    p->radius_min = 1e-32;
    p->radius_max = 1e16;
    p->mu_rel = 1e-12;
    p->mu_rel_max = 1;
    p->tol_fun = 1e-8;
    p->max_iter = lm.max_iter;
    p->max_fun_ev = lm.max_fun_ev;
    p->max_trials = 0;
    p->verbose = 0;
}

} // extern "C"
