// Host-only planner of deferred frames (tc_render_poses): how a list of n_frames frames is cut into launch groups that
// fit the scratch of `capacity` frames that tc_env_reserve_poses sized.  Pure arithmetic on host values, in the style of
// plan_call (tc_plan.h): no HIP header, no device call, so the host compiler builds it alone (tests/test_render_poses_cpu.py
// does) and the host side of the library launches exactly what is tested there.
//
// Group g draws the frames first .. first + count - 1 of the list: one launch of the pose-row kernel (one lane per frame,
// `pose_blocks` workgroups of `pose_nt` lanes) and one frame launch of `count` workgroups, ONE grid row whose width is the
// group (the frame kernels return for blockIdx.x >= N and N is set to `count`, so no slot beyond the list exists).  The
// groups follow each other on the caller's stream and reuse the scratch; a group is never longer than the capacity.
#pragma once

struct PoseGroup {
  long long first;  // first frame of the group in the list
  int count;        // frames of the group: 1 .. capacity
  int pose_blocks;  // workgroups of the pose-row launch
};
// launches a list of n_frames frames takes with a scratch of `capacity` frames (0 for an empty list or no scratch)
static inline long long pose_group_count(long long n_frames, long long capacity) {
  if (n_frames < 1 || capacity < 1) return 0;
  return (n_frames + capacity - 1) / capacity;
}
// group g of them, 0 <= g < pose_group_count
static inline PoseGroup pose_group_at(long long n_frames, long long capacity, long long g, int pose_nt) {
  PoseGroup p;
  p.first = g * capacity;
  const long long left = n_frames - p.first;
  p.count = (int)(left < capacity ? left : capacity);
  p.pose_blocks = (p.count + pose_nt - 1) / pose_nt;
  return p;
}
// the largest capacity a reservation may have: a frame launch is one grid row (2^31 - 1 workgroups), and the slot index
// times the bytes of a draw list stays far inside 64 bits
#define TC_POSES_MAX_CAPACITY 0x7fffffffll
