// Test driver of K41's host mirror (tests/test_sift_gpu.py): ReadImages -> InitImagePairs (CONTIGUOUS) -> MatchImagePairs on the grey images of a file.
//   pvlm_sift_driver <images.bin> <n> <rows> <cols> <num_sift> <root_sift 0|1> <ratio> <matches_threshold> <out.bin>
// images.bin: n images of rows x cols bytes.  out.bin, all little-endian: per frame in id order int64 keypoints, the keypoint records (24 B), the descriptor rows
// (128 floats); then int64 pairs kept, per pair int64 first, second, matches and the (int32 query, int32 train) of every match.
// Also checked here, exit 1 when one fails: ReadImages makes one device call per group of frames; ExtractSIFTHost of every image equals the frame ReadImages filled;
// Frame::ExtractKeyPoints / ComputeDescriptor of one image equal it too, in one device call; RootSIFT over plain descriptors equals the RootSIFT rows; ExtractSIFTQuadtree refuses a depth other than 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

static bool same(const std::vector<KeyPoint>& a, const std::vector<KeyPoint>& b) {
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(KeyPoint)));
}
static bool same(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * 4)); }

int main(int argc, char** argv) {
  try {
    if (argc != 10) { fprintf(stderr, "usage: pvlm_sift_driver images.bin n rows cols num_sift root_sift ratio matches_threshold out.bin\n"); return 2; }
    const int n = std::atoi(argv[2]), rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), num_sift = std::atoi(argv[5]);
    const bool root = std::atoi(argv[6]) != 0;
    const float ratio = (float)std::atof(argv[7]);
    const int threshold = std::atoi(argv[8]);
    std::vector<GrayImage> imgs((size_t)n);
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    for (GrayImage& im : imgs) {
      im.rows = rows; im.cols = cols; im.pixels.resize((size_t)rows * cols);
      if (fread(im.pixels.data(), 1, im.pixels.size(), f) != im.pixels.size()) { fprintf(stderr, "short read\n"); fclose(f); return 2; }
    }
    fclose(f);
    // frames handed over in reverse id order: ReadImages works and leaves them in id order
    std::vector<Frame> frames((size_t)n);
    for (int i = 0; i < n; ++i) { frames[(size_t)i].id = n - 1 - i; frames[(size_t)i].rows = rows; frames[(size_t)i].cols = cols; }
    size_t asked = 0;
    const GrayImageProvider provider = [&](size_t frame, GrayImage& image) { ++asked; image = imgs[(size_t)frames[frame].id]; return true; };
    const long calls0 = SiftDeviceCalls();
    if (!ReadImages(frames, provider, GrayImage(), num_sift, root, 3)) { fprintf(stderr, "ReadImages refused its input\n"); return 1; }
    int bad = 0;
    const long groups = (n + 2) / 3;
    if (SiftDeviceCalls() - calls0 != groups) { fprintf(stderr, "ReadImages made %ld device calls for %ld groups\n", SiftDeviceCalls() - calls0, groups); ++bad; }
    if (asked != (size_t)n) { fprintf(stderr, "the provider was asked %zu times for %d frames\n", asked, n); ++bad; }
    for (int i = 0; i < n; ++i) {
      const Frame& fr = frames[(size_t)i];
      if (fr.id != i || fr.keypoints.size() != fr.keypoints_all.size() || fr.descriptor.size() != fr.keypoints_all.size() * 128 || !fr.img_gray.empty()) { fprintf(stderr, "frame %d: layout\n", i); ++bad; }
      for (size_t k = 0; k < fr.keypoints.size(); ++k) if (fr.keypoints[k][0] != fr.keypoints_all[k].x || fr.keypoints[k][1] != fr.keypoints_all[k].y) { ++bad; break; }
      std::vector<KeyPoint> hk; std::vector<float> hd;
      ExtractSIFTHost(imgs[(size_t)i], GrayImage(), num_sift, root, hk, hd, 8);
      if (!same(hk, fr.keypoints_all) || !same(hd, fr.descriptor)) { fprintf(stderr, "frame %d: ExtractSIFTHost differs from ReadImages\n", i); ++bad; }
    }
    {
      Frame one; one.rows = rows; one.cols = cols; one.img_gray = imgs[0];
      const long calls1 = SiftDeviceCalls();
      const bool a = one.ExtractKeyPoints(num_sift, GrayImage()), b = one.ComputeDescriptor(root);
      if (SiftDeviceCalls() - calls1 != 1) { fprintf(stderr, "ExtractKeyPoints + ComputeDescriptor made %ld device calls\n", SiftDeviceCalls() - calls1); ++bad; }
      if (a != !frames[0].keypoints_all.empty() || b != a || !same(one.keypoints_all, frames[0].keypoints_all) || !same(one.descriptor, frames[0].descriptor)) {
        fprintf(stderr, "Frame::ExtractKeyPoints / ComputeDescriptor differ from ReadImages\n"); ++bad;
      }
      std::vector<float> plain;
      ComputeSIFTDescriptor(imgs[0], one.keypoints_all, plain, false);
      RootSIFT(plain);
      std::vector<float> rooted;
      ComputeSIFTDescriptor(imgs[0], one.keypoints_all, rooted, true);
      if (!same(plain, rooted)) { fprintf(stderr, "RootSIFT over the plain rows differs from the RootSIFT rows\n"); ++bad; }
      std::vector<KeyPoint> none;
      if (ExtractSIFTQuadtree(imgs[0], none, 1, num_sift, GrayImage()) || !none.empty()) { fprintf(stderr, "ExtractSIFTQuadtree served depth 1\n"); ++bad; }
      if (ExtractSIFT(imgs[0], none, 0, GrayImage())) { fprintf(stderr, "ExtractSIFT served num_sift 0\n"); ++bad; }
    }
    std::vector<MatchPair> pairs;
    if (!InitImagePairs(frames, CONTIGUOUS, pairs)) { fprintf(stderr, "InitImagePairs gave no pair\n"); return 1; }
    const size_t listed = pairs.size();
    if (!MatchImagePairs(frames, pairs, ratio, threshold)) { fprintf(stderr, "MatchImagePairs refused its input\n"); return 1; }
    FILE* o = fopen(argv[9], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[9]); return 2; }
    for (const Frame& fr : frames) {
      const long long m = (long long)fr.keypoints_all.size();
      fwrite(&m, 8, 1, o);
      fwrite(fr.keypoints_all.data(), sizeof(KeyPoint), (size_t)m, o);
      fwrite(fr.descriptor.data(), 4, (size_t)m * 128, o);
    }
    const long long np = (long long)pairs.size();
    fwrite(&np, 8, 1, o);
    for (const MatchPair& p : pairs) {
      const long long h[3] = {(long long)p.image_pair.first, (long long)p.image_pair.second, (long long)p.matches.size()};
      fwrite(h, 8, 3, o);
      for (const auto& m : p.matches) { const int qt[2] = {m.first, m.second}; fwrite(qt, 4, 2, o); }
    }
    fclose(o);
    printf("frames %d pairs listed %zu kept %lld checks failed %d\n", n, listed, np, bad);
    return bad ? 1 : 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "pvlm_sift_driver: %s\n", e.what());
    return 1;
  }
}
