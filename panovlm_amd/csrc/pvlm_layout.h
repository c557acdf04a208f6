// Byte layouts of the staging and result buffers of the LiDAR feature front end (K16-K27), each from ONE walk: the function that places the regions also yields the
// size to ask for, so a region cannot end behind the buffer.  Plain C++ (no HIP): tests/cpp/layout_check.cpp writes every region end to end under a sanitizer.
#pragma once
#include <algorithm>
#include <cstddef>

struct pvlm_layout {            // byte layout of one buffer: add() returns the region's offset, bytes is the size to ask for
  size_t bytes = 0;
  size_t add(size_t n, size_t align = 256) { const size_t o = (bytes + align - 1) & ~(align - 1); bytes = o + n; return o; }
};

// Pinned results of a ring batch (pvlm_ring.hip).  Per point: source, ring_col, curvature, half, range, order (4 B each) and, with picks, state (1 B); per (scan,
// ring, sector) a flag; with picks per (scan, ring) the two pick lists (corner_ints / flat_ints ints), the voxel span (8 B) and the ring flag, then voxel_cap
// centroids (16 B).  The raw points go up through the front of the same buffer (16 B each) before any result comes down.
struct pvlm_ring_layout { size_t source, ring_col, curvature, half, range, order, sector, state, corner, flat, voxel_span, ring_host, voxels, bytes; };
inline pvlm_ring_layout pvlm_ring_layout_of(size_t n_points, size_t n_scans, size_t rings, bool picks, size_t corner_ints, size_t flat_ints, size_t voxel_cap) {
  pvlm_layout w; pvlm_ring_layout L{};
  const size_t slots = n_scans * rings;
  L.source = w.add(n_points * 4, 64); L.ring_col = w.add(n_points * 4, 64); L.curvature = w.add(n_points * 4, 64); L.half = w.add(n_points * 4, 64);
  L.range = w.add(n_points * 4, 64); L.order = w.add(n_points * 4, 64); L.sector = w.add(slots * 6, 64);
  if (picks) {
    L.state = w.add(n_points, 64); L.corner = w.add(slots * corner_ints * 4, 64); L.flat = w.add(slots * flat_ints * 4, 64);
    L.voxel_span = w.add(slots * 8, 64); L.ring_host = w.add(slots, 64); L.voxels = w.add(voxel_cap * 16, 64);
  }
  L.bytes = std::max(w.bytes, n_points * 16);
  return L;
}

// Line growth (pvlm_linegrow.hip).  Pinned input: xyz (float4) | point -> scan | scan table.  Pinned output: counters (4 ints) | statuses | segments | members;
// the segment records hold doubles: 8-byte aligned whatever the number of scans.
struct pvlm_grow_in_layout { size_t xyz, pt_scan, scans, bytes; };
struct pvlm_grow_out_layout { size_t counters, status, segs, members, bytes; };
inline pvlm_grow_in_layout pvlm_grow_in_layout_of(size_t n_points, size_t n_scans, size_t scan_bytes) {
  pvlm_layout w; pvlm_grow_in_layout L{};
  L.xyz = w.add(n_points * 16, 16); L.pt_scan = w.add(n_points * 4, 4); L.scans = w.add(n_scans * scan_bytes, 16); L.bytes = w.bytes;
  return L;
}
inline pvlm_grow_out_layout pvlm_grow_out_layout_of(size_t n_scans, size_t seg_cap, size_t seg_bytes, size_t mem_cap) {
  pvlm_layout w; pvlm_grow_out_layout L{};
  L.counters = w.add(16, 4); L.status = w.add(n_scans * 4, 4); L.segs = w.add(seg_cap * seg_bytes, 8); L.members = w.add(mem_cap * 4, 4); L.bytes = w.bytes;
  return L;
}

// Undistort staging (pvlm_undistort.hip): points (float4) | sweep descriptors.
struct pvlm_undistort_layout { size_t points, desc, bytes; };
inline pvlm_undistort_layout pvlm_undistort_layout_of(size_t n_points, size_t n_scans, size_t desc_bytes) {
  pvlm_layout w; pvlm_undistort_layout L{};
  L.points = w.add(n_points * 16); L.desc = w.add(n_scans * desc_bytes); L.bytes = w.bytes;
  return L;
}
