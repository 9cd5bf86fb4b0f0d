// tr_mnl_resident.h — the resident multinomial fit (tr_mnl_resident.hip): one workgroup on one CU
// holds X, the factors and the Adam state in LDS and runs whole fit_Adam iterations per launch; a
// grid of such workgroups fits one independent model each (k_mnl_resident_many).  The carve, the
// argument block and the member table are in tr_mnl_resident_table.h (host code, no HIP).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tr_mnl_resident_table.h"

namespace tr {

hipError_t prepare_resident();
hipError_t launch_resident(const ResArgs& a, const float* X, int64_t xld, const int64_t* target, float* params,
                           const float* w, float* m, float* v, float* vmax, double* loss_hist, int32_t* stop,
                           hipStream_t st);
// One workgroup per row of the device table `members`; lds_bytes is the largest carve among them.
hipError_t launch_resident_many(const ResMember* members, int n_members, int64_t lds_bytes, hipStream_t st);
hipError_t touch_code_object_mnl_resident();

}  // namespace tr
