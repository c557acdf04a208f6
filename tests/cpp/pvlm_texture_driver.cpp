// Test driver of the coloured LiDAR map (Texture::ColorizeLidarPointCloud / FuseCloud, Velodyne::SegmentBatch, SavePCDFileBinary of PointXYZRGB) in the C++
// host mirror.  Commands:
//   texture <pairs.bin> <out.bin> min_dist max_dist skip [map.pcd]
//        pairs.bin: int32 count; per pair int32 scan pose valid, R_wl (9 f64), t_wl (3 f64), int32 name length + name (a .pcd file), int32 frame pose valid,
//        R_wc (9 f64), t_wc (3 f64), int32 rows, int32 cols, rows x cols x 3 BGR bytes.  out.bin: per pair int64 m + m x 4 f32 (cloud_scan of the scan loaded
//        and segmented scan by scan on the host: LoadLidar, ReOrderVLP, Segmentation; 0 points for a scan with an invalid pose), int64 k + k x 16 bytes
//        (GetColoredLidar()[i] as x y z + colour word); then int64 f + f x 16 bytes (FuseCloud(skip)).  map.pcd: the fused cloud through SavePCDFileBinary.
//   segment <scans.bin> <out.bin> num_threads
//        scans.bin: int32 count; per scan int32 mode (0: raw, 1: invalid, 2: already re-ordered), int32 rings, int32 horizon, int32 n + n x 4 f32 (raw cloud).
//        out.bin: per scan int64 m + m x 4 f32 twice: cloud_scan after ReOrderVLP() + Segmentation() scan by scan (an invalid scan: untouched), and after
//        Velodyne::SegmentBatch over all scans.
//   savepcd <records.bin> <out.pcd>        records.bin: int64 n + n x 16 bytes (x y z + colour word); prints "saved 0|1"
//   diverge                                 the two deliberate divergences of Texture; prints "size_mismatch_throws 0|1" and "negative_skip_throws 0|1"
//   texbench <raw_scans.bin> n_pairs n_images rows cols reps
//        raw_scans.bin: tests/host_io.py::write_raw_scans.  Times pvlm_colorize_scans on n_pairs pairs (scan k % count, copied; image k % n_images of a pool
//        of synthetic frames) against a C++ restatement of upstream's per-pair loop (whole-image HSV, and HSV at the hit pixels only) on 1 and 16 threads;
//        prints "key value" lines.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host.hpp"
#include "../../panovlm_amd/csrc/pvlm_texture_core.h"

using namespace pvlm;

template <typename T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), (std::streamsize)(sizeof(T) * n)); }
template <typename T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(sizeof(T) * n)); }

static void WriteCloud(std::ofstream& o, const PointCloud& c) {
  const int64_t n = (int64_t)c.size();
  wr(o, &n, 1);
  if (n) wr(o, &c[0].x, 4 * c.size());
}

static void WriteColored(std::ofstream& o, const std::vector<PointXYZRGB>& c) {
  const int64_t n = (int64_t)c.size();
  wr(o, &n, 1);
  for (const PointXYZRGB& p : c) {
    const uint32_t w = ColourWord(p);
    wr(o, &p.x, 3); wr(o, &w, 1);
  }
}

struct PairIn {
  bool scan_valid = true, frame_valid = true;
  Matrix3d R_wl{}, R_wc{};
  Vector3d t_wl{}, t_wc{};
  std::string name;
  PointCloud cloud_scan;            // texbench
  ColorImage image;
};

static std::vector<PairIn> ReadPairs(const char* path, bool with_clouds) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  int32_t n = 0; rd(f, &n, 1);
  std::vector<PairIn> p((size_t)n);
  for (PairIn& q : p) {
    int32_t v = 0, len = 0;
    rd(f, &v, 1); q.scan_valid = v != 0; rd(f, q.R_wl.data(), 9); rd(f, q.t_wl.data(), 3);
    rd(f, &len, 1); q.name.assign((size_t)len, '\0'); if (len) f.read(&q.name[0], len);
    if (with_clouds) { int32_t m = 0; rd(f, &m, 1); q.cloud_scan.resize((size_t)m); if (m) rd(f, &q.cloud_scan[0].x, 4 * (size_t)m); }
    rd(f, &v, 1); q.frame_valid = v != 0; rd(f, q.R_wc.data(), 9); rd(f, q.t_wc.data(), 3);
    rd(f, &q.image.rows, 1); rd(f, &q.image.cols, 1);
    q.image.bgr.resize((size_t)q.image.rows * q.image.cols * 3);
    if (!q.image.bgr.empty()) rd(f, q.image.bgr.data(), q.image.bgr.size());
  }
  if (!f) throw std::runtime_error(std::string("short file ") + path);
  return p;
}

static void MakeSensors(const std::vector<PairIn>& in, std::vector<Velodyne>& lidars, std::vector<Frame>& frames) {
  lidars.assign(in.size(), Velodyne());
  frames.assign(in.size(), Frame());
  for (size_t i = 0; i < in.size(); ++i) {
    Velodyne& l = lidars[i];
    l.id = (int)i; l.name = in[i].name;
    if (in[i].scan_valid) l.SetPose(in[i].R_wl, in[i].t_wl);
    Frame& fr = frames[i];
    fr.id = (int)i; fr.R_wc = in[i].R_wc; fr.t_wc = in[i].t_wc; fr.pose_valid = in[i].frame_valid;
    fr.rows = in[i].image.rows; fr.cols = in[i].image.cols;
  }
}

static double Seconds(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// upstream's per-pair loop (mvs/Texture.cpp:43-77) in plain C++: the whole image to HSV first (cvtColor), or the HSV of the hit pixels only
static size_t HostPairView(const PointCloud& cloud_scan, const ColorImage& image, const double* T, double min_dist, double max_dist, bool whole_image,
                           std::vector<unsigned char>& hsv, std::vector<PointXYZRGB>& out) {
  const int rows = image.rows, cols = image.cols;
  const unsigned char* img = image.bgr.data();
  if (whole_image) {
    hsv.resize(image.bgr.size());
    for (size_t k = 0; k < (size_t)rows * cols; ++k) {
      int h, s, v;
      pvlm_texture::bgr2hsv_u8(img[3 * k], img[3 * k + 1], img[3 * k + 2], &h, &s, &v);
      hsv[3 * k] = (unsigned char)h; hsv[3 * k + 1] = (unsigned char)s; hsv[3 * k + 2] = (unsigned char)v;
    }
  }
  out.clear();
  const double sq_min = min_dist * min_dist, sq_max = max_dist * max_dist;
  for (const PointXYZI& pt : cloud_scan) {
    int x, y;
    if (!pvlm_texture::project(T, rows, cols, pt.x, pt.y, pt.z, sq_min, sq_max, &x, &y)) continue;
    const size_t k = (size_t)y * cols + x;
    int h, s, v;
    if (whole_image) { h = hsv[3 * k]; s = hsv[3 * k + 1]; v = hsv[3 * k + 2]; }
    else pvlm_texture::bgr2hsv_u8(img[3 * k], img[3 * k + 1], img[3 * k + 2], &h, &s, &v);
    if (pvlm_texture::is_sky(h, s, v)) continue;
    PointXYZRGB c; c.x = pt.x; c.y = pt.y; c.z = pt.z; c.b = img[3 * k]; c.g = img[3 * k + 1]; c.r = img[3 * k + 2];
    out.push_back(c);
  }
  return out.size();
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s texture|segment|savepcd|diverge|texbench ...\n", argv[0]); return 2; }
  const std::string cmd = argv[1];
  try {
    if (cmd == "texture" && argc >= 7) {
      const std::vector<PairIn> in = ReadPairs(argv[2], false);
      std::vector<Velodyne> lidars; std::vector<Frame> frames;
      MakeSensors(in, lidars, frames);
      const double min_dist = atof(argv[4]), max_dist = atof(argv[5]);
      const int skip = atoi(argv[6]);
      Config config; config.num_threads = 16;
      Texture tex(lidars, frames, config, [&](size_t i, ColorImage& im) { im = in[i].image; return true; });
      tex.images_per_call = 3;                                     // several device calls
      tex.ColorizeLidarPointCloud(min_dist, max_dist);
      const std::vector<PointXYZRGB> fused = tex.FuseCloud(skip);
      std::ofstream o(argv[3], std::ios::binary);
      for (size_t i = 0; i < in.size(); ++i) {
        Velodyne v;
        v.name = in[i].name;
        if (in[i].scan_valid) { v.LoadLidar(v.name); if (v.valid) { v.ReOrderVLP(); v.Segmentation(); } }
        WriteCloud(o, v.cloud_scan);
        WriteColored(o, tex.GetColoredLidar()[i]);
      }
      WriteColored(o, fused);
      if (argc > 7) printf("saved %d\n", SavePCDFileBinary(argv[7], fused) ? 1 : 0);
      printf("points %zu\n", fused.size());
    } else if (cmd == "segment" && argc >= 5) {
      std::ifstream f(argv[2], std::ios::binary);
      if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
      int32_t n = 0; rd(f, &n, 1);
      std::vector<Velodyne> a((size_t)n), b;
      for (Velodyne& v : a) {
        int32_t mode = 0, rings = 0, horizon = 0, m = 0;
        rd(f, &mode, 1); rd(f, &rings, 1); rd(f, &horizon, 1); rd(f, &m, 1);
        v.N_SCANS = rings; v.horizon_scans = horizon;
        v.cloud.resize((size_t)m);
        if (m) rd(f, &v.cloud[0].x, 4 * (size_t)m);
        if (mode == 1) v.valid = false;
        if (mode == 2) v.ReOrderVLP();
      }
      b = a;
      for (Velodyne& v : a) if (v.valid) { v.ReOrderVLP(); v.Segmentation(); }
      std::vector<Velodyne*> ptr;
      for (Velodyne& v : b) ptr.push_back(&v);
      Velodyne::SegmentBatch(ptr, atoi(argv[4]));
      std::ofstream o(argv[3], std::ios::binary);
      for (int s = 0; s < n; ++s) { WriteCloud(o, a[(size_t)s].cloud_scan); WriteCloud(o, b[(size_t)s].cloud_scan); }
      printf("scans %d\n", n);
    } else if (cmd == "savepcd" && argc >= 4) {
      std::ifstream f(argv[2], std::ios::binary);
      if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
      int64_t n = 0; rd(f, &n, 1);
      std::vector<PointXYZRGB> c((size_t)n);
      for (PointXYZRGB& p : c) {
        uint32_t w = 0;
        rd(f, &p.x, 3); rd(f, &w, 1);
        p.b = (unsigned char)(w & 255u); p.g = (unsigned char)((w >> 8) & 255u); p.r = (unsigned char)((w >> 16) & 255u);
      }
      printf("saved %d\n", SavePCDFileBinary(argv[3], c) ? 1 : 0);
    } else if (cmd == "diverge") {
      std::vector<Velodyne> two(2);
      std::vector<Frame> one(1);
      int mismatch = 0, negative = 0;
      try { Texture t(two, one, Config()); t.ColorizeLidarPointCloud(1.5, 35); } catch (const std::invalid_argument&) { mismatch = 1; }
      try { Texture t(std::vector<Velodyne>(1), one, Config()); t.FuseCloud(-1); } catch (const std::invalid_argument&) { negative = 1; }
      printf("size_mismatch_throws %d\nnegative_skip_throws %d\n", mismatch, negative);
    } else if (cmd == "texbench" && argc >= 8) {
      // clouds: the raw scans file of tests/host_io.py::write_raw_scans; pair k: a copy (memory of its own) of scan k % count, image k % n_images of a pool
      // of synthetic frames (a sky band over the top third, a pattern below), T_cl a fixed small rigid offset
      std::ifstream f(argv[2], std::ios::binary);
      if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
      int32_t nb = 0; rd(f, &nb, 1);
      std::vector<PointCloud> base((size_t)nb);
      for (PointCloud& c : base) {
        int32_t id = 0, m = 0; double R[9], t[3];
        rd(f, &id, 1); rd(f, R, 9); rd(f, t, 3); rd(f, &m, 1);
        c.resize((size_t)m); if (m) rd(f, &c[0].x, 4 * (size_t)m);
      }
      const int n_pairs = atoi(argv[3]), n_images = std::max(1, atoi(argv[4])), rows = atoi(argv[5]), cols = atoi(argv[6]), reps = std::max(1, atoi(argv[7]));
      std::vector<ColorImage> pool((size_t)n_images);
      for (int i = 0; i < n_images; ++i) {
        ColorImage& im = pool[(size_t)i];
        im.rows = rows; im.cols = cols; im.bgr.resize((size_t)rows * cols * 3);
        for (int r = 0; r < rows; ++r)
          for (int c = 0; c < cols; ++c) {
            unsigned char* q = &im.bgr[((size_t)r * cols + c) * 3];
            if (r < rows / 3) { q[0] = 235; q[1] = 180; q[2] = 120; continue; }
            q[0] = (unsigned char)(r * 7 + c * 3 + 11 * i); q[1] = (unsigned char)((r * 3) ^ (c * 5 + i * 17)); q[2] = (unsigned char)(c + 2 * r + 31 * i);
          }
      }
      std::vector<PairIn> in((size_t)n_pairs);
      std::vector<std::array<double, 12>> T((size_t)n_pairs);
      std::vector<pvlm_colorize_pair> desc((size_t)n_pairs);
      long long total = 0;
      for (int k = 0; k < n_pairs; ++k) {
        PairIn& p = in[(size_t)k];
        p.cloud_scan = base[(size_t)(k % nb)];
        T[(size_t)k] = {0.9998, -0.0175, 0.0087, 0.12, 0.0174, 0.9998, 0.0052, -0.05, -0.0088, -0.0050, 0.9999, 0.21};
        const ColorImage& im = pool[(size_t)(k % n_images)];
        desc[(size_t)k] = pvlm_colorize_pair{&p.cloud_scan[0].x, (int)p.cloud_scan.size(), 4, T[(size_t)k].data(), im.bgr.data(), im.rows, im.cols, 3ll * im.cols};
        total += (long long)p.cloud_scan.size();
      }
      const double min_dist = 1.5, max_dist = 35;
      Engine& e = Engine::Default();
      std::vector<float> rec((size_t)total * 4);
      long long kept = 0;
      e.Check(pvlm_colorize_scans(e.ctx(), n_pairs, desc.data(), min_dist, max_dist, rec.data(), total, &kept, nullptr), "pvlm_colorize_scans");   // warm-up
      std::vector<double> ms;
      for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        e.Check(pvlm_colorize_scans(e.ctx(), n_pairs, desc.data(), min_dist, max_dist, rec.data(), total, &kept, nullptr), "pvlm_colorize_scans");
        ms.push_back(1e3 * Seconds(t0));
      }
      std::sort(ms.begin(), ms.end());
      printf("pairs %d\npoints %lld\nkept %lld\ndevice_call_best_ms %.3f\ndevice_call_median_ms %.3f\n", n_pairs, total, kept, ms[0], ms[ms.size() / 2]);
      // upstream's loop: the hit-pixel form over every pair; the whole-image form (a cvtColor of every frame) over every pair on 16 threads and over the
      // first `sub` pairs on 1 thread (scaled to the set)
      const int sub = std::min(n_pairs, 16);
      for (int whole = 0; whole <= 1; ++whole) {
        for (int threads : {1, 16}) {
          const int np = (whole && threads == 1) ? sub : n_pairs;
          std::atomic<int> next{0};
          std::atomic<size_t> kept_all{0};
          const auto t0 = std::chrono::steady_clock::now();
          std::vector<std::thread> pool_t;
          for (int t = 0; t < threads; ++t) pool_t.emplace_back([&]() {
            std::vector<unsigned char> hsv; std::vector<PointXYZRGB> out;
            for (int i = next++; i < np; i = next++) {
              const ColorImage& im = pool[(size_t)(i % n_images)];
              kept_all += HostPairView(in[(size_t)i].cloud_scan, im, T[(size_t)i].data(), min_dist, max_dist, whole != 0, hsv, out);
            }
          });
          for (std::thread& t : pool_t) t.join();
          const double t_ms = 1e3 * Seconds(t0) * ((double)n_pairs / np);
          const char* form = whole ? "whole_image" : "hit_pixels";
          printf("host_%s_%dthreads_ms %.3f\nhost_%s_%dthreads_pairs_timed %d\nhost_%s_%dthreads_kept %zu\n", form, threads, t_ms, form, threads, np, form, threads,
                 kept_all.load());
        }
      }
    } else {
      fprintf(stderr, "unknown command or missing arguments: %s\n", cmd.c_str());
      return 2;
    }
  } catch (const std::exception& ex) {
    fprintf(stderr, "%s\n", ex.what());
    return 3;
  }
  return 0;
}
