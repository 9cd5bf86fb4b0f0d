// tr_mnl_score.h — the scoring sweep of the multinomial modules (tr_mnl_score.hip): one workgroup per
// (member, row block) runs the forward pass of a (model, data set) pair and forms its probabilities,
// argmax, confusion counts and data loss.  The image, the argument checks and the member table are in
// tr_mnl_score_table.h (host code, no HIP).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tr_mnl_score_table.h"

namespace tr {

hipError_t prepare_score();
// The table's members on `total_blocks` workgroups; lds_bytes is the largest image among them.  The
// counts are zeroed first when any member asks for them, the loss partials added up afterwards when
// any member asks for its loss: up to three launches on `st`.
hipError_t launch_score_many(const ScoreMember* members, int n_members, int64_t total_blocks, int64_t lds_bytes,
                             bool any_counts, bool any_loss, hipStream_t st);

}  // namespace tr
