// Test driver of the fused LiDAR map (LidarOdometry::FuseLidar / CameraLidarOptimizer::FuseLidar, SavePCDFileBinary) in the C++ host mirror.  Commands:
//   fuse <scans.bin> <out.bin> odometry|joint skip min_range max_range [map.pcd]
//        scans.bin: int32 count; per scan int32 valid, R_wl (9 f64), t_wl (3 f64), int32 name length + name, int32 n + n x 4 f32 (cloud),
//        int32 m + m x 4 f32 (cloud_scan).  out.bin: int64 n + n x 4 f32, the fused map.  map.pcd: the map through SavePCDFileBinary as well.
//   savepcd <cloud.bin> <out.pcd>         cloud.bin: int64 n + n x 4 f32; prints "saved 0|1"
//   fusebench <raw_scans.bin> n_scans skip min_range max_range reps
//        raw_scans.bin: tests/host_io.py::write_raw_scans; scan k of the batch is a copy (memory of its own) of file scan k % count with its pose.  Times
//        pvlm_fuse_scans on the scans FuseLidar(skip, ..) visits — into one caller buffer reused across calls, and into a fresh buffer per call — against a
//        plain C++ restatement of upstream's loop on 1 and on 16 threads (scans split across the threads; a fresh result per call, as upstream returns one),
//        and LidarOdometry::FuseLidar itself (a fresh PointCloud per call); prints "key value" lines.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../panovlm_amd/host/pvlm_host.hpp"

using namespace pvlm;

template <typename T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), (std::streamsize)(sizeof(T) * n)); }

static void ReadCloud(std::ifstream& f, PointCloud& c) {
  int32_t n = 0; rd(f, &n, 1);
  c.resize((size_t)n);
  if (n) rd(f, &c[0].x, 4 * (size_t)n);
}

static void WriteCloud(const std::string& path, const PointCloud& c) {
  std::ofstream o(path, std::ios::binary);
  const int64_t n = (int64_t)c.size();
  o.write(reinterpret_cast<const char*>(&n), 8);
  o.write(reinterpret_cast<const char*>(c.data()), (std::streamsize)(c.size() * sizeof(PointXYZI)));
}

static double Seconds(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// upstream's loop body on the scans [s0, s1) as written (PCL's push_back / transformPointCloud / operator+= in plain C++)
static void HostFuse(const std::vector<PointCloud>& clouds, const std::vector<Matrix4d>& poses, size_t s0, size_t s1, double min_range, double max_range,
                     PointCloud& fused) {
  const double sq_min_range = min_range * min_range, sq_max_range = max_range * max_range;
  for (size_t i = s0; i < s1; ++i) {
    PointCloud cloud_filtered;
    for (const PointXYZI& pt : clouds[i]) {
      double range = pt.x * pt.x + pt.y * pt.z + pt.z * pt.z;
      if (range > sq_max_range || range < sq_min_range) continue;
      cloud_filtered.push_back(pt);
    }
    const Matrix4d& T = poses[i];
    for (PointXYZI& p : cloud_filtered) {
      const double x = p.x, y = p.y, z = p.z;
      p.x = (float)(T[0] * x + T[1] * y + T[2] * z + T[3]);
      p.y = (float)(T[4] * x + T[5] * y + T[6] * z + T[7]);
      p.z = (float)(T[8] * x + T[9] * y + T[10] * z + T[11]);
    }
    fused.insert(fused.end(), cloud_filtered.begin(), cloud_filtered.end());
  }
}

static bool SameBits(const PointCloud& a, const PointCloud& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) {
    const float u[4] = {a[i].x, a[i].y, a[i].z, a[i].intensity}, v[4] = {b[i].x, b[i].y, b[i].z, b[i].intensity};
    for (int k = 0; k < 4; ++k) if (!(std::isnan(u[k]) && std::isnan(v[k])) && std::memcmp(&u[k], &v[k], 4) != 0) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s fuse|savepcd|fusebench ...\n", argv[0]); return 2; }
  const std::string cmd = argv[1];
  try {
    if (cmd == "fuse" && argc >= 8) {
      std::ifstream f(argv[2], std::ios::binary);
      if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
      int32_t ns = 0; rd(f, &ns, 1);
      std::vector<Velodyne> l((size_t)ns);
      for (int s = 0; s < ns; ++s) {
        Velodyne& v = l[(size_t)s];
        int32_t valid = 0; rd(f, &valid, 1);
        Matrix3d R; Vector3d t; rd(f, R.data(), 9); rd(f, t.data(), 3);
        int32_t len = 0; rd(f, &len, 1);
        std::string name((size_t)len, '\0');
        if (len) f.read(&name[0], len);
        v.id = s; v.valid = valid != 0; v.name = name; v.SetPose(R, t);
        ReadCloud(f, v.cloud); ReadCloud(f, v.cloud_scan);
      }
      const std::string which = argv[4];
      const int skip = atoi(argv[5]);
      const double min_range = atof(argv[6]), max_range = atof(argv[7]);
      PointCloud map;
      if (which == "odometry") {
        LidarOdometry odo(l, Config());
        map = odo.FuseLidar(skip, min_range, max_range);
      } else if (which == "joint") {
        const Matrix4d T_cl = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        CameraLidarOptimizer opt(T_cl, l, std::vector<Frame>(), Config());
        map = opt.FuseLidar(skip, min_range, max_range);
      } else {
        fprintf(stderr, "unknown class %s\n", which.c_str());
        return 2;
      }
      WriteCloud(argv[3], map);
      if (argc > 8) printf("saved %d\n", SavePCDFileBinary(argv[8], map) ? 1 : 0);
      printf("points %zu\n", map.size());
    } else if (cmd == "savepcd" && argc >= 4) {
      std::ifstream f(argv[2], std::ios::binary);
      if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
      int64_t n = 0; rd(f, &n, 1);
      PointCloud c((size_t)n);
      if (n) rd(f, &c[0].x, 4 * (size_t)n);
      printf("saved %d\n", SavePCDFileBinary(argv[3], c) ? 1 : 0);
    } else if (cmd == "fusebench" && argc >= 8) {
      std::ifstream f(argv[2], std::ios::binary);
      if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
      int32_t nb = 0; rd(f, &nb, 1);
      std::vector<PointCloud> base((size_t)nb);
      std::vector<Matrix4d> base_pose((size_t)nb);
      for (int s = 0; s < nb; ++s) {
        int32_t id = 0; rd(f, &id, 1);
        double R[9], t[3]; rd(f, R, 9); rd(f, t, 3);
        base_pose[(size_t)s] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
        ReadCloud(f, base[(size_t)s]);
      }
      const int n_scans = atoi(argv[3]), skip = atoi(argv[4]), reps = std::max(1, atoi(argv[7]));
      const double min_range = atof(argv[5]), max_range = atof(argv[6]);
      if (nb < 1 || skip < 0) { fprintf(stderr, "fusebench: no scans / skip < 0\n"); return 2; }
      std::vector<Velodyne> l((size_t)n_scans);
      for (int s = 0; s < n_scans; ++s) {
        const Matrix4d& T = base_pose[(size_t)(s % nb)];
        l[(size_t)s].id = s;
        l[(size_t)s].SetPose({T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, {T[3], T[7], T[11]});
        l[(size_t)s].cloud = base[(size_t)(s % nb)];
      }
      // the scans FuseLidar(skip, ..) visits (all valid here), as the plain loops and the device call see them
      std::vector<PointCloud> clouds; std::vector<Matrix4d> poses;
      for (size_t i = 0; i < l.size(); i += (size_t)skip + 1) { clouds.push_back(l[i].cloud); poses.push_back(l[i].GetPose()); }
      long long total = 0;
      std::vector<pvlm_fuse_scan> descs(clouds.size());
      for (size_t k = 0; k < clouds.size(); ++k) {
        const float* p = &clouds[k][0].x;
        descs[k] = pvlm_fuse_scan{p, p + 3, (int)clouds[k].size(), 4, poses[k].data()};
        total += (long long)clouds[k].size();
      }
      printf("scans %zu\npoints_in %lld\n", clouds.size(), total);
      Engine& e = Engine::Default();
      PointCloud dev_out((size_t)total);
      long long kept = 0;
      std::vector<double> t_dev, t_dev_fresh, t_host1, t_host16, t_mirror;
      for (int r = 0; r <= reps; ++r) {                                     // r = 0: warm-up (code objects, pinned window, pool)
        const auto t0 = std::chrono::steady_clock::now();
        e.Check(pvlm_fuse_scans(e.ctx(), (int)descs.size(), descs.data(), min_range, max_range, &dev_out[0].x, total, &kept, nullptr), "pvlm_fuse_scans");
        if (r) t_dev.push_back(Seconds(t0));
      }
      dev_out.resize((size_t)kept);
      printf("points_kept %lld\n", kept);
      // every timing below produces a FRESH result, as upstream's FuseLidar returns one: the page faults of its memory are part of the time (the
      // result is released after the clock stops)
      for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<PointXYZI[]> buf(new PointXYZI[(size_t)total]);   // uninitialised: first touched by the call's copy-out
        e.Check(pvlm_fuse_scans(e.ctx(), (int)descs.size(), descs.data(), min_range, max_range, &buf[0].x, total, &kept, nullptr), "pvlm_fuse_scans");
        t_dev_fresh.push_back(Seconds(t0));
      }
      PointCloud host1, host16;
      for (int r = 0; r < std::min(reps, 3); ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        PointCloud fused;
        HostFuse(clouds, poses, 0, clouds.size(), min_range, max_range, fused);
        t_host1.push_back(Seconds(t0));
        host1 = std::move(fused);
      }
      const size_t n_thr = 16;
      for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<PointCloud> part(n_thr);
        std::vector<std::thread> th;
        for (size_t k = 0; k < n_thr; ++k)
          th.emplace_back([&, k]() { HostFuse(clouds, poses, clouds.size() * k / n_thr, clouds.size() * (k + 1) / n_thr, min_range, max_range, part[k]); });
        for (std::thread& x : th) x.join();
        PointCloud fused;
        for (const PointCloud& p : part) fused.insert(fused.end(), p.begin(), p.end());
        t_host16.push_back(Seconds(t0));
        host16 = std::move(fused);
      }
      for (int r = 0; r < reps; ++r) {
        LidarOdometry odo(l, Config());
        const auto t0 = std::chrono::steady_clock::now();
        const PointCloud m = odo.FuseLidar(skip, min_range, max_range);
        t_mirror.push_back(Seconds(t0));
        if (m.size() != (size_t)kept) { fprintf(stderr, "FuseLidar kept %zu, the call %lld\n", m.size(), kept); return 4; }
      }
      auto best = [](std::vector<double> v) { return *std::min_element(v.begin(), v.end()); };
      auto median = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
      printf("device_call_best_ms %.4f\ndevice_call_median_ms %.4f\n", 1e3 * best(t_dev), 1e3 * median(t_dev));
      printf("device_call_fresh_output_ms %.4f\n", 1e3 * best(t_dev_fresh));
      printf("host_1_thread_ms %.4f\nhost_16_threads_ms %.4f\n", 1e3 * best(t_host1), 1e3 * best(t_host16));
      printf("mirror_fuselidar_ms %.4f\n", 1e3 * best(t_mirror));
      printf("match_host_1 %d\nmatch_host_16 %d\n", SameBits(dev_out, host1) ? 1 : 0, SameBits(dev_out, host16) ? 1 : 0);
    } else {
      fprintf(stderr, "unknown command or missing arguments: %s\n", cmd.c_str());
      return 2;
    }
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 3;
  }
  return 0;
}
