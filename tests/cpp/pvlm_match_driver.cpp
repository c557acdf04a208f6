// Test driver of K33's host mirror (tests/test_match_gpu.py): the matches are made from the descriptors, never handed in.
//   pvlm_match_driver IN OUT ratio matches_threshold
//       MatchImagePairs(frames, pairs, ratio, matches_threshold) on the GPU, MatchImagePairsHost on a copy of the list, then TriangulateTracks(frames, pairs)
// IN:  int32 n_frames, rows, cols, n_pairs; per frame: int32 valid, double R_wc[9], t_wc[3], int32 n_kp, float kp[2 n_kp], float descriptor[128 n_kp];
//      per pair: int32 first, second
// OUT: int32 ok, host_equal, n_pairs; per pair: int32 first, second, n_matches, int32 (queryIdx, trainIdx)[2 n_matches]; int32 n_tracks;
//      per track: uint32 id, double point[3], int32 n_features, uint32 (frame, keypoint)[2 n_features]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

template <typename T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T))); }
template <typename T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T))); }

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s IN OUT ratio matches_threshold\n", argv[0]); return 2; }
  try {
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[4]; rd(f, hdr, 4);
    std::vector<Frame> frames((size_t)hdr[0]);
    for (Frame& fr : frames) {
      int32_t valid = 0, nk = 0;
      rd(f, &valid, 1); rd(f, fr.R_wc.data(), 9); rd(f, fr.t_wc.data(), 3); rd(f, &nk, 1);
      fr.pose_valid = valid != 0; fr.rows = hdr[1]; fr.cols = hdr[2];
      fr.keypoints.resize((size_t)nk); rd(f, reinterpret_cast<float*>(fr.keypoints.data()), 2 * (size_t)nk);
      fr.descriptor.resize(128 * (size_t)nk); rd(f, fr.descriptor.data(), fr.descriptor.size());
    }
    std::vector<MatchPair> pairs((size_t)hdr[3]);
    for (MatchPair& p : pairs) { int32_t h[2]; rd(f, h, 2); p.image_pair = {(size_t)h[0], (size_t)h[1]}; }
    if (!f) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<MatchPair> host_pairs = pairs;
    const float ratio = (float)atof(argv[3]); const int thr = atoi(argv[4]);
    const int32_t ok = MatchImagePairs(frames, pairs, ratio, thr) ? 1 : 0;
    const bool host_ok = MatchImagePairsHost(frames, host_pairs, ratio, thr, 4);
    int32_t host_equal = (host_ok == (ok != 0)) && host_pairs.size() == pairs.size();
    for (size_t p = 0; host_equal && p < pairs.size(); ++p) host_equal = host_pairs[p].image_pair == pairs[p].image_pair && host_pairs[p].matches == pairs[p].matches;
    const std::vector<PointTrack> structure = TriangulateTracks(frames, pairs);
    std::ofstream o(argv[2], std::ios::binary);
    const int32_t head[3] = {ok, host_equal, (int32_t)pairs.size()}; wr(o, head, 3);
    for (const MatchPair& p : pairs) {
      const int32_t h[3] = {(int32_t)p.image_pair.first, (int32_t)p.image_pair.second, (int32_t)p.matches.size()}; wr(o, h, 3);
      for (const auto& m : p.matches) { const int32_t qt[2] = {m.first, m.second}; wr(o, qt, 2); }
    }
    const int32_t nt = (int32_t)structure.size(); wr(o, &nt, 1);
    for (const PointTrack& t : structure) {
      wr(o, &t.id, 1); wr(o, t.point_3d.data(), 3);
      const int32_t nf = (int32_t)t.feature_pairs.size(); wr(o, &nf, 1);
      for (const auto& fp : t.feature_pairs) { const uint32_t v[2] = {fp.first, fp.second}; wr(o, v, 2); }
    }
    return o ? 0 : 1;
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
}
