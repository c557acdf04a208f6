// util/SIFT.cpp:10-128, sensors/Frame.cpp:110-121 and SfM::ReadImages (sfm/SfM.cpp:15-42) on K41: the detection and the batched path through pvlm_sift_extract, the
// one-image descriptor call and ExtractSIFTHost on the host compile of csrc/pvlm_sift_core.h.
#include "pvlm_host_internal.hpp"
#include "../csrc/pvlm_sift_core.h"

namespace pvlm {

namespace {

namespace sf = pvlm_sift;
static_assert(sizeof(KeyPoint) == sizeof(pvlm_sift_keypoint) && sizeof(KeyPoint) == sizeof(sf::Keypoint), "one keypoint record");

bool Usable(const GrayImage& img, const GrayImage& mask) {
  if (img.rows < sf::kMinSide || img.cols < sf::kMinSide || img.pixels.size() != (size_t)img.rows * img.cols) return false;
  return mask.empty() || (mask.rows == img.rows && mask.cols == img.cols && mask.pixels.size() == img.pixels.size());
}

std::atomic<long> g_device_calls{0};

// ONE pvlm_sift_extract call on images of one size.  A call that fails for capacity has done everything but the descriptors, so the buffers are sized before it:
// num_sift keypoints per image (retainBest's bound up to ties) plus kTieRoom, a num_sift above kGuessPerImage (a caller who wants everything) counted as that.  Only
// when more come back (PVLM_ERR_CAPACITY) is the call repeated, with the count it reported.  desc == nullptr: the keypoints alone, no descriptor kernel.
constexpr long long kTieRoom = 64, kGuessPerImage = 1 << 15;
void ExtractBatch(const std::vector<const unsigned char*>& images, int rows, int cols, const GrayImage& mask, int num_sift, bool root_sift, std::vector<long long>& off,
                  std::vector<KeyPoint>& kps, std::vector<float>* desc) {
  Engine& e = Engine::Default();
  off.assign(images.size() + 1, 0);
  const unsigned flags = root_sift ? PVLM_FLAG_SIFT_ROOT : 0u;
  const unsigned char* m = mask.empty() ? nullptr : mask.pixels.data();
  long long capacity = (long long)images.size() * (std::min<long long>(num_sift, kGuessPerImage) + kTieRoom), needed = 0;
  std::vector<float> rows128;
  for (int attempt = 0; attempt < 2; ++attempt) {
    kps.assign((size_t)capacity, KeyPoint{});
    if (desc) rows128.assign((size_t)capacity * 128, 0.f);
    ++g_device_calls;
    const pvlm_status st = pvlm_sift_extract(e.ctx(), (int)images.size(), rows, cols, images.data(), m, num_sift, flags, off.data(), (pvlm_sift_keypoint*)kps.data(),
                                             desc ? rows128.data() : nullptr, capacity, &needed, nullptr);
    if (st != PVLM_ERR_CAPACITY || attempt == 1) { e.Check(st, "pvlm_sift_extract"); break; }
    capacity = needed;
  }
  kps.resize((size_t)needed);
  if (desc) { rows128.resize((size_t)needed * 128); desc->swap(rows128); }
}

void SetPoints(Frame& f) {
  f.keypoints.clear();
  for (const KeyPoint& k : f.keypoints_all) f.keypoints.push_back({k.x, k.y});
}

}  // namespace

long SiftDeviceCalls() { return g_device_calls.load(); }

bool ExtractSIFT(const GrayImage& img_gray, std::vector<KeyPoint>& keypoints, const int num_sift, const GrayImage& mask) {
  if (num_sift <= 0 || !Usable(img_gray, mask)) return false;
  StageTimer stage_timer_("ExtractSIFT");
  std::vector<long long> off;
  ExtractBatch({img_gray.pixels.data()}, img_gray.rows, img_gray.cols, mask, num_sift, false, off, keypoints, nullptr);
  return keypoints.size() > 0;
}

bool ExtractSIFTQuadtree(const GrayImage& img_gray, std::vector<KeyPoint>& keypoints, const int tree_depth, const int num_sift, const GrayImage& mask) {
  if (tree_depth != 0 || num_sift <= 0 || !Usable(img_gray, mask)) return false;
  std::vector<KeyPoint> sub;
  ExtractSIFT(img_gray, sub, num_sift, mask);
  keypoints.insert(keypoints.end(), sub.begin(), sub.end());
  return true;
}

bool ComputeSIFTDescriptor(const GrayImage& img_gray, std::vector<KeyPoint>& keypoints, std::vector<float>& descriptor, const bool root_sift) {
  descriptor.clear();
  if (!Usable(img_gray, GrayImage())) return false;
  sf::Pyramid P;
  const size_t threads = pvlm_thread_cap();
  sf::build_pyramid(img_gray.pixels.data(), img_gray.rows, img_gray.cols, P, threads);
  std::vector<sf::Keypoint> k(keypoints.size());
  if (!k.empty()) std::memcpy(k.data(), keypoints.data(), k.size() * sizeof(KeyPoint));
  descriptor.assign(k.size() * 128, 0.f);
  sf::describe_host(P, k, root_sift, descriptor.data(), threads);
  return !k.empty();
}

void RootSIFT(std::vector<float>& descriptor) {
  for (size_t r = 0; r + 128 <= descriptor.size(); r += 128) {
    float l1 = 0.f;
    for (int k = 0; k < 128; ++k) l1 = l1 + descriptor[r + k];
    if (l1 == 0.f) continue;
    for (int k = 0; k < 128; ++k) descriptor[r + k] = sqrtf(descriptor[r + k] / l1) * 512.f;
  }
}

bool ExtractSIFTHost(const GrayImage& img_gray, const GrayImage& mask, const int num_sift, const bool root_sift, std::vector<KeyPoint>& keypoints,
                     std::vector<float>& descriptor, const int num_threads) {
  keypoints.clear(); descriptor.clear();
  if (num_sift <= 0 || !Usable(img_gray, mask)) return false;
  std::vector<sf::Keypoint> k;
  sf::extract_host(img_gray.pixels.data(), img_gray.rows, img_gray.cols, mask.empty() ? nullptr : mask.pixels.data(), num_sift, root_sift, k, descriptor,
                   (size_t)std::max(1, num_threads));
  keypoints.resize(k.size());
  if (!k.empty()) std::memcpy(keypoints.data(), k.data(), k.size() * sizeof(KeyPoint));
  return !k.empty();
}

// ExtractSIFTQuadtree(img_gray, keypoints_all, 0, num_keypoints, mask) as one device call that also returns the plain descriptor rows: the pyramid is there, and
// ComputeDescriptor would otherwise have to build it again
bool Frame::ExtractKeyPoints(int num_keypoints, const GrayImage& mask) {
  sift_rows.clear();
  if (num_keypoints <= 0 || !Usable(img_gray, mask)) return false;
  const bool fresh = keypoints_all.empty();
  std::vector<long long> off; std::vector<KeyPoint> sub; std::vector<float> rows128;
  ExtractBatch({img_gray.pixels.data()}, img_gray.rows, img_gray.cols, mask, num_keypoints, false, off, sub, &rows128);
  keypoints_all.insert(keypoints_all.end(), sub.begin(), sub.end());                       // upstream appends
  if (fresh) sift_rows.swap(rows128);
  SetPoints(*this);
  return true;
}

bool Frame::ComputeDescriptor(bool root_sift) {
  if (!keypoints_all.empty() && sift_rows.size() == keypoints_all.size() * 128) {          // the rows of ExtractKeyPoints' call; RootSIFT as upstream applies it, afterwards
    descriptor = sift_rows;
    if (root_sift) RootSIFT(descriptor);
    return true;
  }
  return ComputeSIFTDescriptor(img_gray, keypoints_all, descriptor, root_sift);
}

bool ReadImages(std::vector<Frame>& frames, GrayImageProvider images, const GrayImage& mask, const int num_sift, const bool root_sift, const int images_per_call) {
  StageTimer stage_timer_("ReadImages");
  if (num_sift <= 0 || !images || frames.empty()) return false;
  std::vector<size_t> order(frames.size());
  std::iota(order.begin(), order.end(), (size_t)0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return frames[a].id < frames[b].id; });
  const size_t per_call = (size_t)std::max(1, images_per_call);
  struct Result { std::vector<KeyPoint> kps; std::vector<float> desc; };
  std::vector<Result> results(frames.size());
  int rows = 0, cols = 0;
  for (size_t g0 = 0; g0 < order.size(); g0 += per_call) {
    const size_t g1 = std::min(order.size(), g0 + per_call);
    std::vector<GrayImage> imgs(g1 - g0);
    std::vector<const unsigned char*> ptrs;
    for (size_t i = g0; i < g1; ++i) {
      GrayImage& im = imgs[i - g0];
      if (!images(order[i], im)) return false;
      if (g0 == 0 && i == 0) { rows = im.rows; cols = im.cols; }
      if (im.rows != rows || im.cols != cols || !Usable(im, mask)) return false;           // upstream assumes one resolution for all images
      ptrs.push_back(im.pixels.data());
    }
    std::vector<long long> off; std::vector<KeyPoint> kps; std::vector<float> desc;
    ExtractBatch(ptrs, rows, cols, mask, num_sift, root_sift, off, kps, &desc);
    for (size_t i = g0; i < g1; ++i) {
      Result& r = results[order[i]];
      r.kps.assign(kps.begin() + off[i - g0], kps.begin() + off[i - g0 + 1]);
      r.desc.assign(desc.begin() + off[i - g0] * 128, desc.begin() + off[i - g0 + 1] * 128);
    }
  }
  std::vector<Frame> sorted;
  for (size_t i : order) {
    Frame& f = frames[i];
    f.keypoints_all.swap(results[i].kps); f.descriptor.swap(results[i].desc);
    SetPoints(f);
    f.img_gray = GrayImage(); f.sift_rows.clear();                                                              // ReleaseImageGray
    sorted.push_back(std::move(f));
  }
  frames.swap(sorted);                                                                     // sorted by id, as upstream leaves them
  return frames.size() > 0;
}

}  // namespace pvlm
