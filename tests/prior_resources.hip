// Instantiates k_prior (csrc/ba_prior.hip.h) for the register report of tests/test_prior_checks.py -- TEST INFRASTRUCTURE ONLY:
// launch_prior's three instantiations per scalar type (the trial part, the linearisation part without and with the mask) and
// k_prior_lonely's two.
#include "ba_prior.hip.h"

#define BA_PRIOR_INST(T, L, M)                                                                                                              \
    template __global__ void k_prior<T, L, M>(ba_prior_args<T>, int, int, const T *, const T *, T *, T *, T *, T *, T *, T *, T *, const int *, \
                                              const unsigned short *, const unsigned char *);
BA_PRIOR_INST(double, false, false)
BA_PRIOR_INST(double, true, false)
BA_PRIOR_INST(double, true, true)
BA_PRIOR_INST(float, false, false)
BA_PRIOR_INST(float, true, false)
BA_PRIOR_INST(float, true, true)
template __global__ void k_prior_lonely<double, false>(int, const int *, int, const double *, const double *, const double *, const double *, double *, double *, double *, int, const unsigned char *);
template __global__ void k_prior_lonely<double, true>(int, const int *, int, const double *, const double *, const double *, const double *, double *, double *, double *, int, const unsigned char *);
template __global__ void k_prior_lonely<float, false>(int, const int *, int, const float *, const float *, const float *, const float *, float *, float *, float *, int, const unsigned char *);
template __global__ void k_prior_lonely<float, true>(int, const int *, int, const float *, const float *, const float *, const float *, float *, float *, float *, int, const unsigned char *);
