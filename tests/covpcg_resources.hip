// Instantiates the multi-column PCG kernels (csrc/ba_pcg_multi.hip.h) for the register report of tests/test_covariance_pcg_cpu.py -- TEST INFRASTRUCTURE ONLY.
#include "ba_pcg_multi.hip.h"

// (k_mc_prec_inv, k_mc_rhs_cam, k_mc_rhs_pts, k_mc_init, k_mc_update, k_mc_get_cams and k_mc_get_pts are no templates: the header defines them)
template __global__ void k_mc_scal<true>(int, int, const double *, const double *, double, ba_mc_dev *);
template __global__ void k_mc_scal<false>(int, int, const double *, const double *, double, ba_mc_dev *);
template __global__ void k_mc_point<true>(int, const int *, const int *, const double *, const double *, const double *, const double *, const double *,
                                          const ba_mc_dev *, double *);
template __global__ void k_mc_point<false>(int, const int *, const int *, const double *, const double *, const double *, const double *, const double *,
                                           const ba_mc_dev *, double *);
template __global__ void k_mc_cam_chunks<true>(int, const int *, const int *, const int *, const double *, const double *, double *, const ba_mc_dev *);
template __global__ void k_mc_cam_chunks<false>(int, const int *, const int *, const int *, const double *, const double *, double *, const ba_mc_dev *);
#define BA_MC_CAM(F, R)                                                                                                                             \
    template __global__ void k_mc_cam<F, R>(int, const int *, const double *, const double *, const double *, const double *, const double *,     \
                                            const double *, const double *, ba_relpose_csr<double>, const unsigned short *, double *, double *,    \
                                            const ba_mc_dev *);
BA_MC_CAM(true, true)
BA_MC_CAM(true, false)
BA_MC_CAM(false, true)
BA_MC_CAM(false, false)
template __global__ void k_mc_alpha<true>(int, const double *, ba_mc_dev *);
template __global__ void k_mc_alpha<false>(int, const double *, ba_mc_dev *);
