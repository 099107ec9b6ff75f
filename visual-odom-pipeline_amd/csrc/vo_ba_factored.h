// Bundle adjustment, windows of 9 and 10 slots: the FACTORED wave-private build / update (vo_ba_factored.hip), as ba_launch_iter_t of vo_ba.hip
// launches them where the rule (vo_tuning.ba_kernels = 0) took k_ba_build_w<4, 2, 5> / k_ba_update_w<2, 5> before.
#pragma once
#include "vo_ba_dev.h"

// Huber / linear loss, the <4, 2, 5> geometry; grid (G0 * batch) x 256 lanes, dynamic LDS as for k_ba_build_w<4, 2, 5> (vo_ba_ws::v2_lds)
void vo_ba_f_launch_build(dim3 grid, size_t lds, hipStream_t q, const ba_ptrs& P, const ba_params_dev& prm, int it, double probe_lambda, int G0, int Gcap);
void vo_ba_f_launch_update(dim3 grid, hipStream_t q, const ba_ptrs& P, const ba_params_dev& prm, int it, double* probe_dl, int G0, int Gcap);
// the dynamic LDS limit of the build kernel (once per process, ba_alloc)
hipError_t vo_ba_f_set_lds_limits();
