// pvlm_descset (K33): the descriptors of a set of frames, resident on the device.  Created and destroyed by pvlm_match.hip; read by pvlm_vlad.hip (K35).
#pragma once
#include <vector>

#include "pvlm_internal.h"

struct pvlm_descset {
  pvlm_ctx* owner = nullptr;       // the context whose pool holds the arrays: the only one the set may be used with
  int n_frames = 0;
  std::vector<int> rows;
  std::vector<long long> row0;     // first row of every frame in d_desc / d_norm
  std::vector<float> nmax;         // the largest norm2 of every frame
  float* d_desc = nullptr;
  float* d_norm = nullptr;
};
