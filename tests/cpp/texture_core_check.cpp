// Host-compiled check of the per-point statement of K30 (panovlm_amd/csrc/pvlm_texture_core.h: the range test, the transform to the camera, the double
// CamToImage, the rounding, IsInside, OpenCV's 8-bit HSV and the sky test of Texture::ColorizeLidarPointCloud), the functions k_tex_project / k_tex_word_*
// call, driven over caller-given points and pixels so that tests/test_colorize_cpu.py can compare them with the numpy restatement bit for bit on a machine
// without a GPU.  TEST INFRASTRUCTURE ONLY — libpvlm.so has no host path.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared
#include "../../panovlm_amd/csrc/pvlm_texture_core.h"

extern "C" {
// bgr: n x 3; hsv: n x 3
void chk_hsv(const unsigned char* bgr, long long n, unsigned char* hsv) {
  for (long long i = 0; i < n; ++i) {
    int h, s, v;
    pvlm_texture::bgr2hsv_u8(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], &h, &s, &v);
    hsv[3 * i] = (unsigned char)h; hsv[3 * i + 1] = (unsigned char)s; hsv[3 * i + 2] = (unsigned char)v;
  }
}

// int(std::round(v)) with the x86-64 conversion, and IsInside of (x[i], y[i])
void chk_round(const double* v, long long n, int* out) { for (long long i = 0; i < n; ++i) out[i] = pvlm_texture::round_to_int(v[i]); }
void chk_inside(const int* x, const int* y, long long n, int rows, int cols, unsigned char* out) {
  for (long long i = 0; i < n; ++i) out[i] = pvlm_texture::is_inside(x[i], y[i], rows, cols) ? 1 : 0;
}

// pts: n x 3; T: 12 doubles; image: rows x cols x 3 (row_bytes 3 cols).  px / py: the rounded pixel (INT_MIN for NaN), hit: in range and inside,
// word: the record's colour word (0 = dropped)
void chk_colorize(const float* pts, long long n, const double* T, const unsigned char* image, int rows, int cols, double min_dist, double max_dist, int* px,
                  int* py, unsigned char* hit, unsigned* word) {
  const double sq_min = min_dist * min_dist, sq_max = max_dist * max_dist;
  for (long long i = 0; i < n; ++i) {
    const float* p = pts + 3 * i;
    double c[3], u, v;
    pvlm_texture::to_camera(T, p[0], p[1], p[2], c);
    pvlm_equirect::cam_to_image_f64(rows, cols, c[0], c[1], c[2], &u, &v);
    px[i] = pvlm_texture::round_to_int(u); py[i] = pvlm_texture::round_to_int(v);
    int x = 0, y = 0;
    const bool h = pvlm_texture::project(T, rows, cols, p[0], p[1], p[2], sq_min, sq_max, &x, &y);
    hit[i] = h ? 1 : 0;
    word[i] = 0;
    if (h) { const unsigned char* q = image + ((long long)y * cols + x) * 3; word[i] = pvlm_texture::colour_word(q[0], q[1], q[2]); }
  }
}
}
