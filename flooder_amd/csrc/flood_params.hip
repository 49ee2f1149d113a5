// flood_params.hip - the parameter-block entry points (include/flooder_hip.h, "parameter blocks"): the size / abi rule,
// then the launch's own function on the block (flood_common.hpp), which checks the fields and fills the kernels' structs
// from them by name.  The positional exports of the same launches fill a zeroed block and make the same call; nothing
// here touches the device.
#include "../../include/flooder_hip.h"
#include "flood_common.hpp"

using namespace flooder;

extern "C" int flooder_fused_witness(const flooder_fused_sweep_t* p, void* stream) {
  flooder_fused_sweep_t a;
  if (int rc = take(p, a, "flooder_fused_witness: bad parameter block (abi / size)")) return rc;
  return fused_witness(a, stream);
}

extern "C" int flooder_fused_cell(const flooder_fused_sweep_t* p, void* stream) {
  flooder_fused_sweep_t a;
  if (int rc = take(p, a, "flooder_fused_cell: bad parameter block (abi / size)")) return rc;
  return fused_cell(a, stream);
}

extern "C" int flooder_fused_finish(const flooder_fused_sweep_t* p, void* stream) {
  flooder_fused_sweep_t a;
  if (int rc = take(p, a, "flooder_fused_finish: bad parameter block (abi / size)")) return rc;
  return fused_finish(a, stream);
}

extern "C" int flooder_sorted_faces(const flooder_sorted_sweep_t* p, void* stream) {
  flooder_sorted_sweep_t a;
  if (int rc = take(p, a, "flooder_sorted_faces: bad parameter block (abi / size)")) return rc;
  return sorted_sweep(a, SortedMode::faces, stream);
}

extern "C" int flooder_sorted_minima(const flooder_sorted_sweep_t* p, void* stream) {
  flooder_sorted_sweep_t a;
  if (int rc = take(p, a, "flooder_sorted_minima: bad parameter block (abi / size)")) return rc;
  return sorted_sweep(a, a.shard_world > 1 ? SortedMode::shard : SortedMode::minima, stream);
}

extern "C" int flooder_fps_batched(const flooder_fps_batched_t* p, void* stream) {
  flooder_fps_batched_t a;
  if (int rc = take(p, a, "flooder_fps_batched: bad parameter block (abi / size)")) return rc;
  return fps_batched(a, stream);
}
