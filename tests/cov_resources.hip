// Instantiates the covariance kernels (csrc/ba_cov.hip.h) for the register report of tests/test_covariance_cpu.py -- TEST INFRASTRUCTURE ONLY.
#include "ba_cov.hip.h"

template __global__ void k_cov_fixed_records<double>(int, int, int, const int *, const unsigned char *, double *, double *, double *, double *);
template __global__ void k_cov_scale<double>(int, int, const double *, const unsigned short *, double *, int *);
template __global__ void k_cov_stage<double>(int, int, int, const double *, const double *, int, double *);
template __global__ void k_cov_diag<double>(int, int, int, const double *, const double *, double *, int *);
template __global__ void k_cov_syrk<double>(int, int, int, double *, const double *);
template __global__ void k_cov_get_cams<double>(int, const int *, int, const double *, const unsigned short *, double *);
template __global__ void k_cov_points_check<double>(int, int, const int *, const double *, const unsigned char *, const double *, int *);
template __global__ void k_cov_points<double, true>(int, const int *, int, const int *, const int *, const double *, const double *, const unsigned char *,
                                                    double, int, const double *, double *);
template __global__ void k_cov_points<double, false>(int, const int *, int, const int *, const int *, const double *, const double *, const unsigned char *,
                                                     double, int, const double *, double *);
