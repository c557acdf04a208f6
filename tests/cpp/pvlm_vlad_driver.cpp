// Test driver of K35 through the host mirror: VLADMatcher (GenerateCodeBook, ComputeVLADEmbedding, FindNeighbors) on the GPU against the same steps through the host
// loops, InitImagePairs(VLAD | CONTIGUOUS) against InitImagePairsHost, and the pair list through MatchImagePairs.  TEST INFRASTRUCTURE ONLY.
//   pvlm_vlad_driver in.bin out.bin book_size seed
// in:  int32 n_frames; per frame int32 rows, rows x 128 float32.
// out: int32 ok, same_as_host, n_pairs, matched_pairs; n_frames x 3 int32 nearest neighbours; n_pairs x 2 int32 image pairs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host.hpp"

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const int book_size = atoi(argv[3]);
  const unsigned long long seed = strtoull(argv[4], nullptr, 10);
  int n = 0;
  if (fread(&n, 4, 1, in) != 1) return 2;
  std::vector<pvlm::Frame> frames((size_t)n);
  for (int f = 0; f < n; ++f) {
    int rows = 0;
    if (fread(&rows, 4, 1, in) != 1) return 2;
    frames[(size_t)f].id = f;
    frames[(size_t)f].keypoints.assign((size_t)rows, {0.0f, 0.0f});
    frames[(size_t)f].descriptor.resize((size_t)rows * 128);
    if (rows > 0 && fread(frames[(size_t)f].descriptor.data(), 4, (size_t)rows * 128, in) != (size_t)rows * 128) return 2;
  }
  fclose(in);
  int ok = 1, same = 1;
  std::vector<std::vector<size_t>> nb_gpu, nb_host;
  {
    pvlm::VLADMatcher gpu(frames, pvlm::RESIDUAL_NORMALIZATION_PWR_LAW, seed), host(frames, pvlm::RESIDUAL_NORMALIZATION_PWR_LAW, seed, true, 4);
    ok = gpu.GenerateCodeBook(0.5f, book_size) && gpu.ComputeVLADEmbedding() && host.GenerateCodeBook(0.5f, book_size) && host.ComputeVLADEmbedding() ? 1 : 0;
    nb_gpu = gpu.FindNeighbors(3); nb_host = host.FindNeighbors(3);
    if (nb_gpu != nb_host || gpu.GetAlive() != host.GetAlive() || gpu.GetCodeBook().size() != host.GetCodeBook().size()) same = 0;
    else for (size_t k = 0; k < gpu.GetCodeBook().size(); ++k) {
      const float a = gpu.GetCodeBook()[k], b = host.GetCodeBook()[k];
      if (!(a == b)) same = 0;
    }
  }
  std::vector<pvlm::MatchPair> pairs, pairs_host;
  if (!pvlm::InitImagePairs(frames, pvlm::VLAD | pvlm::CONTIGUOUS, pairs, seed, book_size)) ok = 0;
  if (!pvlm::InitImagePairsHost(frames, pvlm::VLAD | pvlm::CONTIGUOUS, pairs_host, seed, book_size, 4)) ok = 0;
  if (pairs.size() != pairs_host.size()) same = 0;
  else for (size_t p = 0; p < pairs.size(); ++p) if (pairs[p].image_pair != pairs_host[p].image_pair) same = 0;
  std::vector<pvlm::MatchPair> gps = pairs;
  if (pvlm::InitImagePairs(frames, pvlm::GPS, gps, seed, book_size) || gps.size() != pairs.size()) ok = 0;     // no GPS in the mirror: false, the list untouched
  std::vector<pvlm::MatchPair> matched = pairs;
  if (!pvlm::MatchImagePairs(frames, matched, 0.8f, 10)) ok = 0;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  const int head[4] = {ok, same, (int)pairs.size(), (int)matched.size()};
  fwrite(head, 4, 4, out);
  for (int f = 0; f < n; ++f)
    for (int k = 0; k < 3; ++k) { const int v = f < (int)nb_gpu.size() && k < (int)nb_gpu[(size_t)f].size() ? (int)nb_gpu[(size_t)f][(size_t)k] : -1; fwrite(&v, 4, 1, out); }
  for (const pvlm::MatchPair& p : pairs) { const int v[2] = {(int)p.image_pair.first, (int)p.image_pair.second}; fwrite(v, 4, 2, out); }
  fclose(out);
  return 0;
}
