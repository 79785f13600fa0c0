// k_poses.h -- deferred frames: from stored poses (x, y, theta and, with camera rows, the row) to the pose rows the frame
// kernels draw from.  A pose row (k_camera.h) is a pure function of (x, y, theta, camera row): cam_pose12 of
// FramePose{x, y, tc_cos(-theta), tc_sin(-theta)} -- tc_cos is exactly even and tc_sin exactly odd, so these are the bits the
// simulate stage hands over, whether it reuses the kinematic update's values or not -- the row's index in entry 12 and
// cam_cull_row's verdict on that very pose in entry TC_CULL_ROW_ENTRY where the handle's rows carry one.  tc_render_poses (the
// host side) runs tc_pose_rows and then the handle's frame kernel with gate = 0 over the rows: the frames are bit for bit what
// the call that produced the poses would have drawn.
// Named without "_kernel": the kernel-variant matrix of the tests keeps a ledger of the tc_*_kernel symbols by family; this one
// stands beside it (tests/test_gpu_render_poses.py).  No template, compiled in part 0.  Includes k_camera.h.
#ifndef K_POSES_H
#define K_POSES_H

#include "k_camera.h"

#define TC_POSES_NT 256

struct PoseArgs {
  KArgs a;                // the handle's arguments: cameras (shared, rows), the cull's table and cover
  const double *x, *y, *theta;  // [n_src]
  const int* camera;      // [n_src] camera row of every pose, or NULL (shared camera: row 0 is never read)
  const long long* index; // [first + n ..] element of the arrays that frame m of the list is drawn from, or NULL = m; clamped into [0, n_src)
  long long n_src;
  long long first;        // frame of the list that lane 0 of the launch draws
  int n;                  // frames of this launch
  int cam_rows;           // rows of a.cam_E / a.cam_K (`camera` is clamped into them); 0 with the shared camera
  double* rows;           // [n][TC_POSE_ROW] out, or NULL
  // handles without a frame kernel: the gathered poses as plain arrays [n] each (read in place of the env's state), or NULL
  double *gx, *gy, *gth;
  int* gcam;
};
// (the argument block through the kernarg segment, as step_args(): cam_pose12 reads the shared camera with scalar loads from
// the address of a.cam.E)
typedef const __attribute__((address_space(4))) PoseArgs* PoseArgsConst;
__device__ __forceinline__ const PoseArgs& pose_args() {
  unsigned long long p = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const PoseArgs*)(PoseArgsConst)p;
}

// One lane per frame.  Plain vector stores: the rows are complete before the frame launch behind this one starts.
TC_PLAIN_KERNEL __global__ __launch_bounds__(TC_POSES_NT) void tc_pose_rows(PoseArgs p_unused) {
  const PoseArgs& p = pose_args();
  const long long m = (long long)blockIdx.x * TC_POSES_NT + threadIdx.x;  // slot of the launch: frame p.first + m of the list
  if (m >= (long long)p.n) return;
  long long j = p.index ? p.index[p.first + m] : p.first + m;
  j = j < 0 ? 0 : (j >= p.n_src ? p.n_src - 1 : j);
  int cam_row = 0;
  if (p.camera) {
    const int c = p.camera[j];
    cam_row = c < 0 ? 0 : (c >= p.cam_rows ? p.cam_rows - 1 : c);
  }
  const double x = p.x[j], y = p.y[j], th = p.theta[j];
  if (p.gx) {
    p.gx[m] = x;
    p.gy[m] = y;
    p.gth[m] = th;
    p.gcam[m] = cam_row;
  }
  if (!p.rows) return;
  FramePose fp;
  fp.x = x;
  fp.y = y;
  fp.cth = tc_cos(-th);  // car.py:159-165
  fp.sth = tc_sin(-th);
  double pose[12];
  cam_pose12(p.a, cam_row, fp, pose);
  double2* o = (double2*)(p.rows + (size_t)m * TC_POSE_ROW);
#pragma unroll
  for (int i = 0; i < 6; i++) o[i] = make_double2(pose[2 * i], pose[2 * i + 1]);
  ((long long*)o)[12] = cam_row;
  if (p.a.cull_rows) ((unsigned long long*)o)[TC_CULL_ROW_ENTRY] = cam_cull_row(p.a, pose);
}

#endif  // K_POSES_H
