// Internal: the opaque dt_handle behind include/dtsim.h, shared by the step
// (dtsim.hip) and observation (dtrender.hip) translation units.
#pragma once
#include <string>
#include <vector>

#include "dtdevbuf.h"
#include "dtrecords.h"
#include "dtrender.h"
#include "dtsim_common.h"

struct StepCfg {
  int32_t repeat, frame_skip, action_mode, clip, speed_measured, auto_reset;
  uint32_t max_steps, max_env_steps, max_spawn_attempts;
  double reward_scale;
};

struct dt_handle {
  int device = 0;
  int n = 0;
  dt_config cfg{};
  dt::Geo geo{};
  StepCfg sc{};
  dt::MapDev map{};
  DevBuf map_buf;
  dt::State st{};
  DevBuf st_buf;
  size_t lds_bytes = 0;     // the map image the kernels stage (walker rows included)
  uint32_t env_base = 0;
  // observation path (dtrender.hip)
  dt_line_params line_params{};
  dr::LineDev line{};
  DevBuf mark_buf;   // float4 segments (x0, z0, x1, z1): yellow then white
  int32_t n_yellow = 0, n_white = 0;
  DevBuf render_spill;           // per env: listed words past the LDS list (dtrender.hip)
  DevBuf render_sched;           // render_kernel's dispatch order state (dtrender.hip)
  uint32_t render_launches = 0;  // dt_render launches (the order's double-buffer parity)
  // the last render launch that used the dispatch-order state: its stream; a
  // render on another stream records the event there and waits for it
  hipEvent_t render_done = nullptr;
  hipStream_t render_stream = nullptr;
  bool render_pending = false;
  // dt_render_objects: the footprint records the render draws (0: none)
  DevBuf render_objs;   // float [DT_MAX_RENDER_OBJECTS][DT_RENDER_OBJ_STRIDE]
  int32_t n_render_objs = 0;
  // dt_render_walkers: a row per record above (0: none walk)
  DevBuf render_walk;   // float [DT_MAX_RENDER_OBJECTS][DT_RENDER_WALK_STRIDE]
  int32_t n_render_walk = 0;
  std::vector<uint8_t> render_walker;   // [n_render_walk]: the record walks (K != 0)
  // dt_set_walkers' packed rows (empty: none) and dt_set_bots' table: the two
  // share the map's mover rows, which set_movers (dtsim.hip) composes
  std::vector<double> walk_rows_host;   // [n_obj][dt::kWalkRec]
  std::vector<int32_t> bot_row;         // [n_bots] rows of dt_map.objects
  DevBuf bot_tab;                       // double [bot_rows][n_bots][DT_OBJ_STRIDE]
  int32_t bot_rows = 0;
  // dt_render_bots: the frame's bot table and each bot's render record (0: none)
  DevBuf render_bot_tab;                // float [rows][n][DT_RENDER_OBJ_STRIDE]
  DevBuf render_bot_col;                // int32 [DT_MAX_RENDER_OBJECTS]: column or -1
  int32_t n_render_bots = 0, render_bot_rows = 0;
  std::vector<int32_t> render_bot_row;  // [n_render_bots] records of dt_render_objects
  // dt_render_camera: the forward view's gather table (on: the kCam kernels run)
  DevBuf render_cam;                    // uint16 [120 * 160], allocated once
  bool render_cam_on = false;
  std::string err;
  // (the caller has made `device` current: dt_destroy, dt_create)
  ~dt_handle() {
    if (render_done) (void)hipEventDestroy(render_done);
  }
};

// Launch entry points run on the handle's GPU whatever the calling thread's
// current device is (a VecEnv on cuda:1 called from a thread whose current
// device is 0); the caller's current device is restored on return.
struct DevGuard {
  int prev = -1;
  explicit DevGuard(int device) {
    if (hipGetDevice(&prev) == hipSuccess && prev != device) {
      if (hipSetDevice(device) != hipSuccess) prev = -1;
    } else {
      prev = -1;
    }
  }
  ~DevGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

// record a failed HIP call in the handle and return DT_E_HIP
#define HIP_OR_FAIL(h, expr)                                                   \
  do {                                                                         \
    if (hip_said((h)->err, #expr, (expr)) != hipSuccess) return DT_E_HIP;      \
  } while (0)

// upload_in_place (dtdevbuf.h) into the handle's `buf`, failing as HIP_OR_FAIL
// does, with its text for the three calls written out
#define UPLOAD_IN_PLACE_OR_FAIL(h, buf, capacity, src, bytes)                  \
  do {                                                                         \
    const UploadCalls _c = {                                                   \
        "hipMalloc(&h->" #buf ", " #capacity ")", "hipDeviceSynchronize()",    \
        "hipMemcpy(h->" #buf ", " #src ", " #bytes ", hipMemcpyHostToDevice)"}; \
    if (upload_in_place((h)->buf, capacity, src, bytes, _c, (h)->err) != hipSuccess) \
      return DT_E_HIP;                                                         \
  } while (0)

// a dtrecords.h check's text: into the handle with DT_E_ARG, DT_OK for none
inline int refused(dt_handle* h, const std::string& why) {
  if (why.empty()) return DT_OK;
  h->err = why;
  return DT_E_ARG;
}

// dtrender.hip: lane-marking polylines of the map + default line params
int dt_render_init(dt_handle* h, const dt_map* map);
