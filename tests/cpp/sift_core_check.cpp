// Host compile of csrc/pvlm_sift_core.h (K41) for the tests: the C entry points below are loaded by tests/sift_ref.py (build/libsift_check.so, -ffp-contract=off);
// with -DSIFT_CHECK_MAIN the file is a stand-alone program that runs the whole-image host loop on seeded images of awkward sizes under the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../panovlm_amd/csrc/pvlm_sift_core.h"

namespace sf = pvlm_sift;

extern "C" {

int chk_sift_sizes(int rows, int cols, int* oct_rows, int* oct_cols) {
  const sf::Sizes s = sf::octave_sizes(rows, cols);
  for (int o = 0; o < s.n_oct; ++o) { oct_rows[o] = s.rows[o]; oct_cols[o] = s.cols[o]; }
  return s.n_oct;
}

void chk_sift_kernels(int* taps, float* coeff /* 6 x 27 */) {
  sf::Kernel K[sf::kGauss];
  sf::make_kernels(K);
  for (int i = 0; i < sf::kGauss; ++i) { taps[i] = K[i].taps; std::memcpy(coeff + i * sf::kMaxTaps, K[i].c, sizeof(K[i].c)); }
}

// the doubled image, 2 rows x 2 cols floats
void chk_sift_doubled(const unsigned char* img, int rows, int cols, float* out) {
  for (int y = 0; y < 2 * rows; ++y) for (int x = 0; x < 2 * cols; ++x) out[(size_t)y * 2 * cols + x] = sf::doubled_at(img, rows, cols, y, x);
}

// the layers of one octave: gauss 6 x R x C, dog 5 x R x C
void chk_sift_pyramid(const unsigned char* img, int rows, int cols, int octave, float* gauss, float* dog) {
  sf::Pyramid P;
  sf::build_pyramid(img, rows, cols, P);
  const size_t n = (size_t)P.sz.rows[octave] * P.sz.cols[octave];
  for (int l = 0; l < sf::kGauss; ++l) std::memcpy(gauss + l * n, P.g(octave, l), n * sizeof(float));
  for (int l = 0; l < sf::kDog; ++l) std::memcpy(dog + l * n, P.d(octave, l), n * sizeof(float));
}

// candidates and keypoints before the selection; counters: extrema, moved, reject_moves, reject_contrast, reject_edge, candidates, multi_peak, keypoints
void chk_sift_detect(const unsigned char* img, int rows, int cols, sf::Cand* cands, long long cand_cap, long long* n_cands, sf::Keypoint* kps, long long kp_cap,
                     long long* n_kps, long long* counters) {
  sf::Pyramid P;
  sf::build_pyramid(img, rows, cols, P);
  std::vector<sf::Cand> c; std::vector<sf::Keypoint> k; sf::Counters ct;
  sf::detect_host(P, c, k, &ct);
  *n_cands = (long long)c.size(); *n_kps = (long long)k.size();
  for (long long i = 0; i < cand_cap && i < *n_cands; ++i) cands[i] = c[(size_t)i];
  for (long long i = 0; i < kp_cap && i < *n_kps; ++i) kps[i] = k[(size_t)i];
  const long long v[8] = {ct.extrema, ct.moved, ct.reject_moves, ct.reject_contrast, ct.reject_edge, ct.candidates, ct.multi_peak, ct.keypoints};
  std::memcpy(counters, v, sizeof(v));
}

// detected_or_null: the keypoints before the selection
long long chk_sift_extract(const unsigned char* img, int rows, int cols, const unsigned char* mask, int nfeatures, int root, sf::Keypoint* kps, float* desc, long long cap,
                           int threads, long long* detected_or_null) {
  std::vector<sf::Keypoint> k; std::vector<float> d; sf::Counters ct;
  sf::extract_host(img, rows, cols, mask, nfeatures, root != 0, k, d, (size_t)(threads > 0 ? threads : 1), &ct);
  if (detected_or_null) *detected_or_null = ct.keypoints;
  const long long n = (long long)k.size();
  for (long long i = 0; i < cap && i < n; ++i) { kps[i] = k[(size_t)i]; std::memcpy(desc + i * sf::kDescBins, d.data() + i * sf::kDescBins, sf::kDescBins * sizeof(float)); }
  return n;
}

long long chk_sift_select(sf::Keypoint* kps, long long n, int nfeatures, int rows, int cols, const unsigned char* mask) {
  std::vector<sf::Keypoint> k(kps, kps + n);
  sf::select(k, nfeatures, rows, cols, mask);
  for (size_t i = 0; i < k.size(); ++i) kps[i] = k[i];
  return (long long)k.size();
}

void chk_sift_desc_finish(const float* hist, int root, float* out) { sf::desc_finish(hist, root != 0, out); }
float chk_sift_atan2_deg(float y, float x) { return sf::atan2_deg(y, x); }
void chk_sift_sincos_deg(float deg, double* s, double* c) { sf::sincos_deg(deg, s, c); }
float chk_sift_pow2(float t) { return sf::pow2_f(t); }

}  // extern "C"

#if defined(SIFT_CHECK_MAIN)
static unsigned g_seed = 12345u;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static void blob_image(int rows, int cols, std::vector<unsigned char>& img) {
  std::vector<float> f((size_t)rows * cols, 40.f);
  const int nb = 6 + (rows * cols) / 400;
  for (int b = 0; b < nb; ++b) {
    const float cy = (float)(rnd() % (unsigned)rows), cx = (float)(rnd() % (unsigned)cols), s = 1.5f + (float)(rnd() % 40u) * 0.1f, a = (b & 1) ? 150.f : -30.f;
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) f[(size_t)y * cols + x] += a * (float)std::exp(-(((float)y - cy) * ((float)y - cy) + ((float)x - cx) * ((float)x - cx)) / (2.f * s * s));
  }
  img.resize(f.size());
  for (size_t i = 0; i < f.size(); ++i) { const float v = f[i] + (float)(rnd() % 5u); img[i] = (unsigned char)(v < 0.f ? 0.f : v > 255.f ? 255.f : v); }
}

int main() {
  const int sizes[][2] = {{8, 8}, {8, 40}, {40, 9}, {17, 33}, {64, 96}, {119, 161}};
  int bad = 0;
  for (const auto& s : sizes)
    for (int variant = 0; variant < 3; ++variant) {
      std::vector<unsigned char> img, mask;
      blob_image(s[0], s[1], img);
      if (variant == 2) { mask.assign(img.size(), 0); for (int y = 0; y < s[0]; ++y) for (int x = 0; x < s[1] / 2; ++x) mask[(size_t)y * s[1] + x] = 1; }
      std::vector<sf::Keypoint> k; std::vector<float> d;
      sf::Counters ct;
      sf::extract_host(img.data(), s[0], s[1], mask.empty() ? nullptr : mask.data(), variant == 1 ? 5 : 100000, variant != 0, k, d, 2, &ct);
      bool ok = d.size() == k.size() * sf::kDescBins;
      for (float v : d) ok = ok && v >= 0.f && v <= 512.f;
      for (const sf::Keypoint& q : k) ok = ok && q.x > -1.f && q.x < (float)s[1] + 1.f && q.y > -1.f && q.y < (float)s[0] + 1.f && q.angle >= 0.f && q.angle < 360.f && q.size > 0.f;
      if (variant == 2) for (const sf::Keypoint& q : k) ok = ok && q.x < (float)(s[1] / 2) + 0.5f;
      printf("%3d x %3d variant %d: extrema %lld candidates %lld keypoints %zu %s\n", s[0], s[1], variant, ct.extrema, ct.candidates, k.size(), ok ? "ok" : "MISMATCH");
      bad += !ok;
    }
  return bad ? 1 : 0;
}
#endif
