// pvlm_depthset (K37 / K39): the uint16 depth maps of a set of frames, resident on the device.  Created, filled, read and destroyed by pvlm_depthfill.hip; read by
// pvlm_scale.hip (K39).  All of its memory comes from the owner's pool, as a pvlm_descset's does: pvlm_mem_info counts it as in use, pvlm_trim cannot take it.
#pragma once
#include <vector>

#include "pvlm_internal.h"

struct pvlm_depthset {
  pvlm_ctx* owner = nullptr;                 // the context whose pool holds the maps: the only one the set may be used with
  int n_frames = 0;
  std::vector<int> rows, cols;               // 0 x 0: the frame has no map (upstream's depth_map.empty())
  std::vector<unsigned short*> d_map;        // rows[f] x cols[f], row-major; null for an empty frame
  unsigned short* d_block = nullptr;         // pvlm_depthset_compute: the ONE allocation every d_map[f] points into
  std::vector<unsigned short*> d_own;        // pvlm_depthset_upload: the frame's own allocation (null where d_map[f] lies in d_block or is empty)
};
