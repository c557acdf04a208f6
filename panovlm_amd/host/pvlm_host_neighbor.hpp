// K49 in the host mirror: MVS::SelectNeighborSFM (mvs/MVS.cpp:248-332) and the dispatch MVS::SelectNeighborViews (:66-79), beside SelectNeighborKNN, which stays as
// it is.  Included at the end of pvlm_host.hpp; defined in pvlm_host_neighbor.cpp.  See pvlm.h (K49) for the definition.
#pragma once

namespace pvlm {

enum NeighborSelection { SFM_POINTS = 1, NEAREST_NEIGHBOR = 2 };          // mvs/MVS.h:32-36

// The neighbours of every view from the triangulated tracks the views share: per track and per i < j of its views the angle factor times the depth-ratio factor into
// a float F x F matrix, then per row the candidates by score descending (equal scores by column descending) until neighbor_size are accepted.  A candidate is
// accepted when ||t_nr|| > sq_distance_threshold: upstream compares the norm, not its square, with the squared threshold (:322), and so does this.  NeighborInfo holds
// R_nr / t_nr as float by the rigid inverse, as SelectNeighborKNN.  host = false: pvlm_mvs_select_neighbors_sfm (the score matrix stays on the device; rows the
// device cannot certify are redone by the literal loop inside the call, stats->n_uncertain of them).  host = true: the literal loop (select_host of
// csrc/pvlm_neighbor_sfm_core.h), which is what the tests compare the device with.  false with `neighbors` holding frames.size() empty lists: an empty structure
// ("SfM points are empty"), or a track that names a frame past frames.size() or one without a valid pose (upstream would read a sentinel pose: the deliberate divergence).
bool SelectNeighborSFM(const std::vector<Frame>& frames, const std::vector<PointTrack>& structure, int neighbor_size, float sq_distance_threshold,
                       std::vector<std::vector<NeighborInfo>>& neighbors, const bool host = false, pvlm_neighbor_sfm_stats* stats = nullptr,
                       std::vector<std::vector<float>>* scores = nullptr);

// MVS::SelectNeighborViews (:66-79): `neighbors` cleared and resized, NEAREST_NEIGHBOR -> SelectNeighborKNN, SFM_POINTS -> SelectNeighborSFM, both with
// Square(min_distance); any other method is false ("Unknown neighbor selection method").
bool SelectNeighborViews(const std::vector<Frame>& frames, const std::vector<PointTrack>& structure, int neighbor_size, int method, float min_distance,
                         std::vector<std::vector<NeighborInfo>>& neighbors, const bool host = false);

}  // namespace pvlm
