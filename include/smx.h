/*
 * smx.h — C-ABI of libsmarts_mi355x.so: the MI355X-native SMARTS hot path.
 *
 * One handle = one GPU = one shard of E independent environment instances x N
 * vehicle slots.  The boundary replaces the seam
 *     SMARTS.step(agent_actions) -> (obs, rewards, dones, scores)
 *                                   reference smarts/core/smarts.py:187-227, 236-327
 *     SMARTS.reset(scenario)     -> first observations
 *                                   reference smarts/core/smarts.py:365-460
 * for a batch of instances, the way ParallelEnv batches whole processes
 * (reference smarts/env/wrappers/parallel_env.py:214-233, 303-309 auto-reset).
 * The reference has no FFI on this path (it imports pybullet/sumolib directly), so
 * the entry points below are what a cffi/ctypes binding of that seam would bind;
 * INTEGRATION.md shows the binding.
 *
 * Conventions: every function returns 0 on success, a negative smx_status on
 * failure and never throws; smx_last_error() gives the text.  The caller owns
 * every device buffer (PyTorch-ROCm tensors handed over as raw pointers); the
 * library allocates only the map tables.  A handle is not thread-safe; distinct
 * handles are independent.  smx_step / smx_reset enqueue work on the given HIP
 * stream and do no host<->device copies and no synchronisation.
 */
#ifndef SMX_H
#define SMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smx_handle_s* smx_handle;

typedef enum smx_status {
  SMX_OK = 0,
  SMX_ERR_INVALID = -1,  /* bad argument / shape / null pointer */
  SMX_ERR_HIP = -2,      /* a HIP runtime call failed */
  SMX_ERR_STATE = -3,    /* call order (e.g. step before load_map) */
  SMX_ERR_NOMEM = -4
} smx_status;

/* ---- action space: reference smarts/core/controllers/__init__.py:42-54, 137-144 ---- */
enum {
  SMX_ACTION_KEEP_LANE = 0,         /* "keep_lane"         -> target 15.0 m/s, lane change 0  */
  SMX_ACTION_SLOW_DOWN = 1,         /* "slow_down"         -> target  0.0 m/s, lane change 0  */
  SMX_ACTION_CHANGE_LANE_LEFT = 2,  /* "change_lane_left"  -> target 12.5 m/s, lane change +1 */
  SMX_ACTION_CHANGE_LANE_RIGHT = 3, /* "change_lane_right" -> target 12.5 m/s, lane change -1 */
  SMX_ACTION_NONE = -1              /* agent sent no action this tick (smarts.py:1233-1240) */
};

/* ---- done criteria bits: reference smarts/core/agent_interface.py:186-206 ---- */
enum {
  SMX_DONE_COLLISION = 1 << 0,
  SMX_DONE_OFF_ROAD = 1 << 1,
  SMX_DONE_OFF_ROUTE = 1 << 2,
  SMX_DONE_ON_SHOULDER = 1 << 3,
  SMX_DONE_WRONG_WAY = 1 << 4,
  SMX_DONE_NOT_MOVING = 1 << 5
};

/* ---- event columns of smx_outputs.events, order of reference smarts/core/events.py:23-34 ---- */
enum {
  SMX_EV_COLLISIONS = 0,
  SMX_EV_OFF_ROAD = 1,
  SMX_EV_OFF_ROUTE = 2,
  SMX_EV_ON_SHOULDER = 3,
  SMX_EV_WRONG_WAY = 4,
  SMX_EV_NOT_MOVING = 5,
  SMX_EV_REACHED_GOAL = 6,
  SMX_EV_REACHED_MAX_EPISODE_STEPS = 7,
  SMX_EV_AGENTS_ALIVE_DONE = 8,
  SMX_EV_COUNT = 9
};

/* ---- sensor switches: reference smarts/core/agent_interface.py:209-297 ---- */
enum {
  SMX_SENSOR_WAYPOINTS = 1 << 0,
  SMX_SENSOR_NEIGHBORS = 1 << 1,
  SMX_SENSOR_ACCELEROMETER = 1 << 2,
  SMX_SENSOR_OGM = 1 << 3,
  SMX_SENSOR_LIDAR = 1 << 4,
  SMX_SENSOR_DAGM = 1 << 5,  /* drivable-area grid map (sensors.py:675-716) */
  SMX_SENSOR_ROAD_WAYPOINTS = 1 << 6, /* RoadWaypointsSensor (sensors.py:991-1040) */
  /* lane_ttc (smarts/env/custom_observations.py:148-280), the observation adapter behind StdObs.ttc
   * (format_obs.py:551-562), computed on the device from this pass's wp_*, nb_* and ego_* rows
   * (smx_outputs.lane_ttc).  Valid only together with SMX_SENSOR_WAYPOINTS and SMX_SENSOR_NEIGHBORS, and while
   * wp_paths * wp_len <= SMX_TTC_MAX_WAYPOINTS (an agent's waypoints are staged in LDS). */
  SMX_SENSOR_LANE_TTC = 1 << 7,
  /* The ego-centric observation adapter (smarts/core/utils/adapters/ego_centric_adapters.py:60-176 over
   * smarts/core/utils/math.py:452-505) on the device: every position and heading of this pass's ego, waypoint,
   * neighbour, lidar and road-waypoint rows (those whose sensors are on) in the frame of the agent's own vehicle,
   * written beside the world rows (smx_outputs.ego_frame, ec_*), and the frame kept for smx_actions_to_world. */
  SMX_SENSOR_EGO_CENTRIC = 1 << 8,
  /* The top-down RGB camera (RGB of agent_interface.py; sensors.py:761-794 over renderer.py:346-395): the OGM's and the
   * DAGM's orthographic camera — centred on the vehicle, up its heading, row 0 ahead — over a black clear colour, with
   * the two substitutions those grids already have.  The image is [rgb_height][rgb_width][3] uint8; pixel centres are
   * the OGM's.  Every pixel gets the HIGHEST class that holds for its centre:
   *   0  none of the below                                                                        bytes   0,   0,   0
   *   1  within half a lane width of a segment of that lane's centre line (the DAGM's test, every
   *      lane, junction-internal lanes included): SceneColors.Road, colors.py:62                  bytes  80,  80,  80
   *   2  inside the chassis rectangle of an alive social vehicle of the env (the OGM's test):
   *      Silver, colors.py:60                                                                     bytes 192, 192, 192
   *   3  inside the chassis rectangle of an alive agent vehicle of the env, the observer included:
   *      SceneColors.Agent, colors.py:58                                                          bytes 210,  30,  30
   * (the vehicles stand above the road; where two vehicles overlap, "agent over social" is this path's rule,
   * DESIGN.md).  The image is not part of smx_outputs: the caller binds its buffer with smx_set_rgb_output.  The image
   * of an agent without an observation in the pass is not written. */
  SMX_SENSOR_RGB = 1 << 9
};
#define SMX_TTC_MAX_WAYPOINTS 512

enum { SMX_SOCIAL_CONSTANT = 0, SMX_SOCIAL_IDM = 1 };

/* ActionSpaceType (controllers/__init__.py:42-57) values on this path.  Lane takes int8 codes
 * (smx_step); the others take three floats per agent (smx_step_continuous):
 *   CONTINUOUS                 throttle, brake, steering                  (:94-99)
 *   ACTUATOR_DYNAMIC           throttle, brake, steering rate             (actuator_dynamic_controller.py:47-80)
 *   LANE_WITH_CONTINUOUS_SPEED target speed, lane change (-1 / 0 / +1), - (:113-124)
 *   IMITATION                  acceleration (m/s^2), angular velocity (rad/s), - (imitation_controller.py:57-78); a NaN
 *                              angular velocity beside a finite first float selects the reference's scalar form: the
 *                              first float is then a speed to set, the pose is held (:50-56)
 * A NaN in the first float means "no action this tick".
 * The values are this interface's own: 7 and 8 follow on, 9 stays invalid (the reference's Python enum has MPC = 7,
 * Imitation = 9; smarts_amd/env/agent_interface.py keeps those). */
enum {
  SMX_ACTION_SPACE_LANE = 0,
  SMX_ACTION_SPACE_CONTINUOUS = 1,
  SMX_ACTION_SPACE_ACTUATOR_DYNAMIC = 2,
  SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED = 3,
  SMX_ACTION_SPACE_TRAJECTORY = 4, /* smx_step_trajectory: PD tracking (trajectory_tracking_controller.py:176-331) */
  /* The kinematic spaces: the agent's vehicle is a box that a provider places (BoxChassis, chassis.py:187-320); no
   * controller, no dynamics model. */
  SMX_ACTION_SPACE_TARGET_POSE = 5,         /* smx_step_target_pose: MotionPlannerProvider + BezierMotionPlanner
                                               (motion_planner_provider.py:65-129, bezier_motion_planner.py:38-121) */
  SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME = 6, /* smx_step_trajectory_with_time: TrajectoryInterpolationProvider
                                                (trajectory_interpolation_provider.py:96-193) */
  SMX_ACTION_SPACE_MPC = 7, /* smx_step_trajectory: the closed-form horizon-5 MPC (trajectory_tracking_controller.py:56-173,
                               476-609), the sedan's mass, yaw inertia and tyre cornering stiffnesses; a dynamic agent */
  SMX_ACTION_SPACE_IMITATION = 8 /* smx_step_continuous: ImitationController on a BoxChassis (imitation_controller.py:30-78;
                                    Imitation is not a dynamic action space in this reference version, smarts.py:163-171,
                                    so the agent is a kinematic one) */
};

#define SMX_MAX_ALIVE_LISTS 4
typedef struct smx_config {
  int32_t num_envs;          /* E: environment instances in this shard            */
  int32_t num_vehicles;      /* N: vehicle slots per instance (<= 64)             */
  double dt;                 /* fixed_timestep_sec, reference hiway_env.py:113    */
  uint32_t sensors;          /* SMX_SENSOR_* bits                                 */
  uint32_t done_criteria;    /* SMX_DONE_* bits                                   */
  int32_t wp_lookahead;      /* Waypoints.lookahead (agent_interface.py:78), 32   */
  int32_t wp_paths;          /* dense rows kept per agent, format_obs.py:42 -> 4  */
  int32_t wp_len;            /* dense waypoints kept per path, format_obs.py:42 -> 20 */
  int32_t nb_max;            /* dense neighbour rows, format_obs.py:41 -> 10      */
  double nb_radius;          /* NeighborhoodVehicles.radius; < 0 = unlimited      */
  int32_t max_episode_steps; /* <= 0 = None                                       */
  /* Device-side frame stacking (FrameStack of smarts/env/wrappers/frame_stack.py over (env, slot) rows): 0 = off,
   * 2..8 = the number of frames kept of every row bound with smx_bind_frame_stack (1 is refused: the reference
   * asserts num_stack > 1).  It takes the four bytes that were padding ahead of not_moving_time: the struct's size
   * and every other offset are unchanged, and a zeroed struct of an older caller reads "off". */
  int32_t frame_stack;
  double not_moving_time;    /* EventConfiguration, agent_interface.py:175-183    */
  double not_moving_distance;
  int32_t auto_reset;        /* ParallelEnv auto_reset, parallel_env.py:303-309   */
  int32_t reset_elapsed_steps; /* ticks the reference spends before the first ego
                                  observation exists (smarts.py:426-434)          */
  int32_t ogm_width, ogm_height; /* OGM sensor grid (agent_interface.py:42-51)    */
  double ogm_resolution;
  int32_t lidar_rays;        /* number of rays in smx_lidar_rays                  */
  double lidar_max_distance;
  int32_t action_space;      /* SMX_ACTION_SPACE_*                                */
  /* Scripted social traffic (stands in for the SUMO provider on fixed-vehicle-count scenarios,
   * smarts.py:868-921, chassis.py:187-320 BoxChassis): the LAST num_social slots of every env
   * are kinematic lane followers.  They move along their lane's centre line at
   * social_speed_factor x the lane's speed limit, continue onto outgoing lane
   * (slot + lanes crossed) mod #outgoing, are seen by every sensor and collision test, and
   * produce no observation of their own.  State reuse: SMX_S_MCL_X = lane, SMX_S_MCL_Y =
   * arclength offset, SMX_S_SPD_INT = lanes crossed. */
  int32_t num_social;
  double social_speed_factor;
  /* DoneCriteria.agents_alive (agent_interface.py:155-176, sensors.py:404-441): an agent is done
   * when fewer agents are left in its env than asked.  Counts are taken over the agents registered
   * at the start of the tick (agent_manager ids).  0 = not set; alive_list_mask[k] bit i = agent
   * slot i belongs to list k (agents_list), alive_list_min[k] = minimum_agents_alive_in_list. */
  int32_t via_max;           /* near-via rows kept per agent (<= 32); 0 = via sensor off */
  int32_t alive_min_ego;
  int32_t alive_min_total;
  int32_t alive_lists;          /* number of lists used, <= SMX_MAX_ALIVE_LISTS */
  int32_t alive_list_min[4];
  uint64_t alive_list_mask[4];
  /* drivable-area grid map (agent_interface.py:29-38): same view as the OGM (centred on the ego,
   * row 0 ahead), 255 where the pixel centre lies within half a lane width of a lane centre line */
  int32_t dagm_width, dagm_height;
  double dagm_resolution;
  /* Speed model of the scripted social vehicles: SMX_SOCIAL_CONSTANT = social_speed_factor x the speed
   * limit; SMX_SOCIAL_IDM = intelligent-driver car following towards that desired speed (accel 2.6,
   * decel 4.5, tau 1.0, min gap 2.5: SUMO's passenger defaults).  The leader is the nearest alive
   * vehicle of the env (agents included) less than 60 m ahead along the follower's heading and less
   * than 1.6 m to its side, read at the start of the tick; gap = centre distance - 3.68.  Parity with
   * SUMO's own car-following is unpinned. */
  int32_t social_model;
  /* RoadWaypointsSensor (agent_interface.py RoadWaypoints.horizon, sensors.py:991-1040): per lane of the nearest
   * lane's road, its parallel roads and the roads oncoming at the vehicle, the waypoint paths of lookahead
   * 2 x horizon that start `horizon` metres behind the vehicle (through incoming lanes where the lane is shorter).
   * Dense rows: the first rw_lanes lanes (<= SMX_RW_LANE_CAP) in the reference's order, the first rw_paths paths
   * of each, 2 x horizon + 1 waypoints per path; true counts are reported beside them. */
  int32_t rw_horizon;        /* 1 .. SMX_RW_HORIZON_MAX; read when SMX_SENSOR_ROAD_WAYPOINTS is set */
  int32_t rw_lanes;
  int32_t rw_paths;
  /* SMX_SENSOR_RGB (agent_interface.py RGB: 256 x 256 at 50 / 256): the grid of the top-down RGB image; width * height
   * a multiple of 16 and at most 65536 (the class tile of one image is staged in LDS) */
  int32_t rgb_width, rgb_height;
  double rgb_resolution;
} smx_config;
#define SMX_RW_LANE_CAP 8
#define SMX_RW_HORIZON_MAX 64

/* ---- packed map records (smarts_amd.map_compiler.pack_tables) ---- */
typedef struct smx_lp_rec {   /* one lanepoint = one 64-byte line (LanePoint + LinkedLanePoint, lanepoints.py:46-70) */
  double x, y, heading;       /* pose (heading as Pose.heading yields it, coordinates.py:394-403) */
  double dirx, diry;          /* radians_to_vec(heading) (math.py:247-253), host libm */
  int32_t lane;
  int32_t next_off;           /* first successor record in succ_rec */
  int32_t next0;              /* first successor lanepoint, -1 none */
  uint16_t n_next;
  uint8_t inferred;           /* LinkedLanePoint.is_inferred */
  uint8_t flags;              /* bit 0: interpolated points down the chain have consecutive indices */
  int32_t knot_next;          /* next non-inferred lanepoint following successor 0 */
  int32_t knot_hops;          /* hops from here to knot_next */
} smx_lp_rec;
typedef struct smx_succ_rec { /* one entry of LinkedLanePoint.nexts */
  int32_t idx;                /* the successor lanepoint */
  int32_t lane;               /* its lane (route filter of lanepoints.py:666-683) */
  int32_t knot;               /* first non-inferred lanepoint down that branch */
  int32_t hops;               /* hops from the branching point to it */
} smx_succ_rec;
typedef struct smx_shape_rec { /* one centre-line vertex of a lane (Lane shape, sumo_road_network.py:287-296) */
  double x, y;
  double cum;                 /* arclength from the lane's first vertex, summed vertex by vertex */
  double len;                 /* length of the segment to the next vertex (0 on the last one)   */
} smx_shape_rec;
typedef struct smx_pt_rec { double x, y; int32_t idx, lane; } smx_pt_rec;   /* lanepoint grid member */
typedef struct smx_seg_rec {  /* centre-line segment grid member */
  double x1, y1, x2, y2;
  double thr;                 /* 0.5 * lane width + 0.1 (road_with_point, sumo_road_network.py:707) */
  double len, cum;            /* shape_rec[v0].len / .cum: the segment's length and its arclength along the lane */
  int32_t lane;
  int32_t v0;                 /* index of the segment's first vertex in shape_rec (its second one is v0 + 1) */
} smx_seg_rec;

/* Host-side map tables produced by smarts_amd.map_compiler (compile_map + pack_tables).
 * smx_load_map copies them to the device.  Lane order = sumolib _allLanes order. */
typedef struct smx_map_tables {
  int32_t n_lanes, n_roads, n_lanepoints, n_shape_pts, n_succ;
  const int32_t* lane_road;
  const int32_t* lane_index;
  const double* lane_width;
  const double* lane_speed;
  const double* lane_length;     /* the net.xml length attribute (sumo_road_network.py:283-285) */
  const uint8_t* lane_in_junction;
  const int32_t* lane_shape_off; /* n_lanes + 1 */
  const double* shape_x;
  const double* shape_y;
  const smx_shape_rec* shape_rec; /* n_shape_pts, same order as shape_x / shape_y */
  const int32_t* lane_out_off;   /* n_lanes + 1 */
  const int32_t* lane_out_idx;   /* Lane.outgoing_lanes (sumo_road_network.py:350-358) */
  const int32_t* road_lane_off;  /* n_roads + 1 */
  const int32_t* road_lanes;
  const uint8_t* road_is_junction;
  const int32_t* road_out_road;
  const smx_lp_rec* lp_rec;      /* n_lanepoints, the reference's global lanepoint order */
  const smx_succ_rec* succ_rec;  /* n_succ */
  double lpg_x0, lpg_y0, lpg_cell; /* uniform grid over lanepoints (replaces scipy KD-trees) */
  int32_t lpg_nx, lpg_ny;
  const int32_t* lpg_off;        /* lpg_nx * lpg_ny + 1 */
  const smx_pt_rec* lpg_pts;     /* members by value, contiguous per cell */
  double sg_x0, sg_y0, sg_cell;  /* uniform grid over centre-line segments (replaces the rtree) */
  int32_t sg_nx, sg_ny;
  const int32_t* sg_off;         /* sg_nx * sg_ny + 1 */
  const smx_seg_rec* sg_rec;
  double default_lane_width;     /* sumo_road_network.py:80 */
  /* RoadWaypointsSensor's neighbourhood (sensors.py:991-1040) */
  const int32_t* lane_in_off;    /* n_lanes + 1 */
  const int32_t* lane_in_idx;    /* Lane.incoming_lanes (sumo_road_network.py:342-348), sumolib's order */
  const int32_t* road_par_off;   /* n_roads + 1 */
  const int32_t* road_par_idx;   /* Road.parallel_roads (sumo_road_network.py:607-618) */
} smx_map_tables;

/* ---- simulation state, caller-owned device memory, struct-of-arrays over (E, N) ---- */
enum {
  SMX_S_X = 0, SMX_S_Y, SMX_S_HEADING,   /* pose of the base frame (chassis.py:493-505) */
  SMX_S_U, SMX_S_V, SMX_S_R,             /* body-frame velocity + yaw rate               */
  SMX_S_DELTA,                            /* steer joint angle (chassis.py:510-525)       */
  SMX_S_LAT_INT, SMX_S_SPD_INT, SMX_S_STEER, SMX_S_THROTTLE, SMX_S_SPD_ERR,
  SMX_S_MCL_X, SMX_S_MCL_Y,              /* LaneFollowingControllerState (lane_following_controller.py:34-49) */
  SMX_S_TRIP_X, SMX_S_TRIP_Y, SMX_S_TRIP_H, SMX_S_DIST, /* TripMeterSensor (sensors.py:880-947) */
  SMX_S_LV0_LONG, SMX_S_LV0_LAT, SMX_S_AV0_Z,           /* AccelerometerSensor history (sensors.py:1046-1087) */
  SMX_S_LV1_LONG, SMX_S_LV1_LAT, SMX_S_AV1_Z,
  SMX_S_PATH_SUM,                        /* DrivenPathSensor running window length (sensors.py:855-877) */
  SMX_S_PREV_X, SMX_S_PREV_Y,            /* position at the previous observation (driven-path segment) */
  SMX_S_COUNT
};
/* Agents of the kinematic action spaces have no dynamics model and no controller; their slots keep the provider's and
 * BoxChassis' state in rows that only those read (as the social slots reuse SMX_S_MCL_X / _Y / SMX_S_SPD_INT):
 *   SMX_S_U       = the provider's speed (VehicleState.speed; SMX_S_V and SMX_S_R stay 0); Imitation: the speed the
 *                   controller hands to BoxChassis.control, which may be negative
 *   SMX_S_DELTA   = TargetPose: the provider's own heading (MotionPlannerProvider._poses[:, 2], never re-normalised,
 *                   motion_planner_provider.py:99), while SMX_S_HEADING holds Heading() of it (:109)
 *   SMX_S_LAT_INT = BoxChassis._last_heading (chassis.py:211-217)
 *   SMX_S_SPD_INT = BoxChassis._last_dt; 0 for a freshly created vehicle (the constructor's control(pose, speed)) */
enum { SMX_S_KIN_RAW_HEADING = SMX_S_DELTA, SMX_S_KIN_LAST_HEADING = SMX_S_LAT_INT, SMX_S_KIN_LAST_DT = SMX_S_SPD_INT };
enum {
  SMX_F_ALIVE = 1 << 0,
  SMX_F_MCL_SET = 1 << 1,
  SMX_F_GUARDED = 1 << 2, /* the state guard has ended this agent (smx_set_guard): done at its next observation; cleared
                             when the slot's vehicle is created again.  Never set while the guard is off. */
  SMX_F_HIST_SHIFT = 3, /* bits 3-4: accelerometer samples held (0..2) */
  SMX_F_FIRST = 1 << 5, /* vehicle was just (re)created: its next observation is a reset observation */
  SMX_F_SOCIAL = 1 << 6, /* scripted social vehicle (no controller, no observation) */
  SMX_F_LEFT = 1 << 7, /* a history agent whose recorded vehicle has left the table (smx_set_history_agents): done at this
                          tick's observation; cleared when the slot's vehicle is created again.  Never set without a binding. */
  SMX_F_ENTERING = 1 << 8 /* beside SMX_F_FIRST: an agent entering inside a tick (smx_set_agent_entry), whose first
                             observation runs its collision test; cleared with SMX_F_FIRST.  Never set without a binding. */
};

#define SMX_DRIVEN_PATH_LEN 500 /* DrivenPathSensor deque, sensors.py:838 */

/* Element types of the caller-owned buffers (the dtype the caller declares for each pointer). */
enum { SMX_DT_NONE = 0, SMX_DT_F64, SMX_DT_F32, SMX_DT_I32, SMX_DT_I16, SMX_DT_I8, SMX_DT_U8, SMX_DT_U64 };
enum { /* indices into smx_state.count / .dtype: the pointers in declaration order */
  SMX_ST_F64 = 0, SMX_ST_FLAGS, SMX_ST_STEPS, SMX_ST_ENV_TICKS, SMX_ST_ENV_DONE_COUNT, SMX_ST_ENV_EPISODE,
  SMX_ST_DRIVEN_PATH, SMX_ST_SEED_CACHE, SMX_ST_FACTS_I32, SMX_ST_FACTS_F64, SMX_ST_ENV_RESET_PENDING,
  SMX_ST_BUFFERS
};
typedef struct smx_state {
  double* f64;        /* [SMX_S_COUNT][E*N]                                    */
  int32_t* flags;     /* [E*N]  SMX_F_* bits                                   */
  int32_t* steps;     /* [E*N]  SensorState._step (sensors.py:609-637)         */
  int32_t* env_ticks; /* [E]    ticks since reset (elapsed_sim_time = ticks*dt)*/
  int32_t* env_done_count; /* [E] agents that have ever been done (hiway_env.py:258-261) */
  int32_t* env_episode;    /* [E] episodes completed (indexes the spawn table) */
  double* driven_path; /* [E*N][SMX_DRIVEN_PATH_LEN] ring of step lengths, or NULL
                         when SMX_DONE_NOT_MOVING tracking is not wanted        */
  int32_t* seed_cache; /* [SMX_SEED_COUNT][E*N]: start road / route filter / start lanepoints
                          found by the last observation at the vehicle's current pose; the
                          next tick's controller queries the map at that same pose
                          (lane_following_controller.py:96-98) and reuses them     */
  int32_t* facts_i32;  /* [SMX_FACT_I_COUNT][E*N] per-tick map facts of each vehicle (scan kernel
                          -> observe kernels): nearest lane, road flags, trip-meter seed   */
  double* facts_f64;   /* [SMX_FACT_F_COUNT][E*N]: nearest-lane distance, lane heading there  */
  int32_t* env_reset_pending; /* [E] set by the observe kernel when auto_reset fires        */
  /* what the caller allocated: element count and SMX_DT_* of each buffer above, in declaration order
   * (SMX_ST_*); checked against the sizes smx_config implies on every entry (smx_check_buffers) */
  uint64_t count[SMX_ST_BUFFERS];
  uint8_t dtype[SMX_ST_BUFFERS + 5]; /* (+5: keeps the struct a multiple of 8 bytes) */
} smx_state;
#define SMX_SEED_COUNT 9 /* road, filter n, filter roads x2, lane count, start lanepoint x4 */
enum {
  SMX_FI_LANE = 0, SMX_FI_FLAGS, SMX_FI_TRIP_START, SMX_FI_OBS_START,
  SMX_FI_TRIP_HAS_WP, /* trip meter holds a waypoint (TripMeterSensor._wps_for_distance non-empty); persists across ticks */
  SMX_FI_FLAGS_NEXT,  /* the flags word after this tick's observation, applied by the commit kernel */
  SMX_FI_VIA_CONSUMED, /* bit v: via v of the agent's list was hit in this episode (ViaSensor._consumed_via_points) */
  SMX_FACT_I_COUNT
};
enum { SMX_FF_LANE_DIST = 0, SMX_FF_LANE_HEADING /* lane heading at the nearest centre-line point */, SMX_FACT_F_COUNT };
enum { SMX_FACT_ON_ROAD = 1 << 0, SMX_FACT_CORNER_SHIFT = 1 /* bits 1-4: corner q on road */ };

/* Spawn table: episode k of env e starts from row (k mod episodes).
 * x, y = vehicle centre, heading in reference convention, speed m/s. */
typedef struct smx_spawns {
  int32_t episodes;
  const double* pose; /* device, [episodes][E*N][4] = x, y, heading, speed */
  const double* social; /* device, [episodes][E*N][2] = lane, arclength offset (social slots only; NULL if none) */
  uint64_t pose_count, social_count; /* float64 elements the caller allocated for each table */
} smx_spawns;

/* ---- per-tick outputs, caller-owned device memory, dense StdObs layout
 *      (reference smarts/env/wrappers/format_obs.py:40-42, 313-373, 401-603) ---- */
enum { /* columns of smx_outputs.ego_f32 */
  SMX_EGO_HEADING = 0, SMX_EGO_SPEED, SMX_EGO_STEERING, SMX_EGO_YAW_RATE,
  SMX_EGO_LIN_VEL = 4,  /* 3 */
  SMX_EGO_ANG_VEL = 7,  /* 3 */
  SMX_EGO_LIN_ACC = 10, /* 3 */
  SMX_EGO_ANG_ACC = 13, /* 3 */
  SMX_EGO_LIN_JERK = 16,/* 3 */
  SMX_EGO_ANG_JERK = 19,/* 3 */
  SMX_EGO_BOX = 22,     /* 3: length, width, height */
  SMX_EGO_F32_COUNT = 25
};

/* ---- columns of smx_outputs.lane_ttc and bits of smx_outputs.lane_ttc_flags: what
 *      lane_ttc(observation) returns (custom_observations.py:148-184); its "speed" and "steering" entries are
 *      ego_f32[SMX_EGO_SPEED] / [SMX_EGO_STEERING] and are not repeated ---- */
enum {
  SMX_TTC_DIST_FROM_CENTER = 0, /* signed lateral error to the closest first waypoint / half its lane width */
  SMX_TTC_ANGLE_ERROR = 1,      /* that waypoint's heading relative to the ego's                             */
  SMX_TTC_TTC = 2,              /* 3: "ego_ttc" of the right, current and left lane                          */
  SMX_TTC_DTC = 5,              /* 3: "ego_lane_dist" of the same lanes                                      */
  SMX_TTC_COUNT = 8
};
enum {
  SMX_TTC_VALID = 1 << 0,       /* the agent has an observation with at least one path: the row was written */
  SMX_TTC_STD = 1 << 1,         /* ... and at least one neighbour: FormatObs' _std_ttc would not be None     */
  /* the dense rows did not hold the sensors' full output (wp_count[0] > wp_paths, nb_count > nb_max or
   * wp_len < wp_lookahead + 1): the row is lane_ttc of the rows that were kept */
  SMX_TTC_TRUNCATED = 1 << 2,
  /* the closest first waypoint's lane_index is not an index into the per-path list (the reference indexes that
   * list by lane index and raises IndexError, custom_observations.py:263): the six lane columns are written as 0 */
  SMX_TTC_INDEX_ERROR = 1 << 3
};

enum { /* indices into smx_outputs.count / .dtype: the pointers in declaration order */
  SMX_OUT_EGO_POS = 0, SMX_OUT_EGO_F32, SMX_OUT_EGO_LANE, SMX_OUT_EVENTS, SMX_OUT_REWARD, SMX_OUT_DIST, SMX_OUT_DONE,
  SMX_OUT_ACTIVE, SMX_OUT_ENV_DONE, SMX_OUT_VIA_NEAR, SMX_OUT_VIA_NEAR_COUNT, SMX_OUT_VIA_HIT, SMX_OUT_LEARNER,
  SMX_OUT_WP_POS, SMX_OUT_WP_HEADING, SMX_OUT_WP_LANE_WIDTH, SMX_OUT_WP_SPEED_LIMIT, SMX_OUT_WP_LANE_INDEX,
  SMX_OUT_WP_LANE_ID, SMX_OUT_WP_COUNT, SMX_OUT_NB_POS, SMX_OUT_NB_BOX, SMX_OUT_NB_HEADING, SMX_OUT_NB_SPEED,
  SMX_OUT_NB_LANE_INDEX, SMX_OUT_NB_LANE_ID, SMX_OUT_NB_SLOT, SMX_OUT_NB_COUNT, SMX_OUT_OGM, SMX_OUT_LIDAR_HIT,
  SMX_OUT_LIDAR_POINT, SMX_OUT_DAGM, SMX_OUT_COLLIDEES,
  SMX_OUT_RW_LANE_COUNT, SMX_OUT_RW_LANE, SMX_OUT_RW_PATH_COUNT, SMX_OUT_RW_COUNT, SMX_OUT_RW_POS, SMX_OUT_RW_HEADING,
  SMX_OUT_RW_LANE_WIDTH, SMX_OUT_RW_SPEED_LIMIT, SMX_OUT_RW_LANE_INDEX, SMX_OUT_RW_LANE_ID,
  SMX_OUT_FINAL_EGO_POS, SMX_OUT_FINAL_EGO_F32, SMX_OUT_FINAL_EGO_LANE, SMX_OUT_FINAL_EVENTS, SMX_OUT_FINAL_DIST,
  SMX_OUT_LANE_TTC, SMX_OUT_LANE_TTC_FLAGS,
  SMX_OUT_EGO_FRAME, SMX_OUT_EC_FLAGS, SMX_OUT_EC_EGO_F32, SMX_OUT_EC_WP_POS, SMX_OUT_EC_WP_HEADING, SMX_OUT_EC_NB_POS,
  SMX_OUT_EC_NB_HEADING, SMX_OUT_EC_LIDAR_POINT, SMX_OUT_EC_RW_POS, SMX_OUT_EC_RW_HEADING,
  SMX_OUT_BUFFERS
};
typedef struct smx_outputs {
  double* ego_pos;       /* [E*N][3]                                          */
  float* ego_f32;        /* [E*N][SMX_EGO_F32_COUNT]                          */
  int16_t* ego_lane;     /* [E*N][2] = lane id (table index, -1 none), lane_index */
  uint8_t* events;       /* [E*N][SMX_EV_COUNT]                               */
  double* reward;        /* [E*N] trip-meter increment (agent_manager.py:233) */
  double* dist;          /* [E*N] distance_travelled / score                  */
  uint8_t* done;         /* [E*N]                                             */
  uint8_t* active;       /* [E*N] 1 while the agent has a vehicle after this tick */
  uint8_t* env_done;     /* [E]   dones["__all__"] (hiway_env.py:258-261)     */
  /* via sensor (if smx_set_vias gave any): the near vias (within the 40 m lane acquisition range,
   * vehicle.py:553-557) as indices into the agent's list, nearest first, -1 padded; bit v of
   * via_hit = via v was hit this tick */
  int8_t* via_near;      /* [E*N][via_max]                                    */
  uint8_t* via_near_count; /* [E*N]                                           */
  int32_t* via_hit;      /* [E*N]                                             */
  /* optional learner-facing block [2][E*N] float32: row 0 = reward, row 1 = done, rewritten whole
   * every tick (absent agents read 0) — what a multi-GPU job gathers per tick;
   * the caller may alternate buffers between ticks.  NULL if unused. */
  float* learner;
  /* waypoints sensor, [E*N][wp_paths][wp_len] */
  double* wp_pos;        /* ...[3], z = 0 (format_obs.py:594)                 */
  float* wp_heading;
  float* wp_lane_width;
  float* wp_speed_limit;
  int8_t* wp_lane_index;
  int16_t* wp_lane_id;   /* extra: lane table index of each waypoint          */
  uint8_t* wp_count;     /* [E*N][wp_paths + 1]: total #paths, then #waypoints per kept path */
  /* neighbourhood sensor, [E*N][nb_max] */
  double* nb_pos;        /* ...[3]                                            */
  float* nb_box;         /* ...[3]                                            */
  float* nb_heading;
  float* nb_speed;
  int8_t* nb_lane_index; /* -1 when no lane within the observer's length      */
  int16_t* nb_lane_id;
  int8_t* nb_slot;       /* vehicle slot of each neighbour, -1 = padding      */
  uint8_t* nb_count;     /* [E*N] neighbours found (may exceed nb_max)        */
  /* occupancy grid sensor [E*N][ogm_height][ogm_width], NULL if unused.
   * These rows are the handle's to maintain between calls: a tile is mostly zeros that stay zeros, so a call stores only the
   * pieces of a tile that are non-zero now or were after the last call (the handle keeps a bit per piece) and the rows
   * read after every call exactly as if whole tiles had been stored.  Reading them is free.  A caller that WRITES into
   * them calls smx_invalidate_outputs before the next call; passing another buffer than the last call's is detected, and
   * either makes that call store whole tiles.  smx_set_ogm_delta(h, 0) stores whole tiles always. */
  uint8_t* ogm;
  /* lidar sensor [E*N][lidar_rays]: hit flag + point, NULL if unused         */
  uint8_t* lidar_hit;
  double* lidar_point;   /* ...[3]                                            */
  /* drivable-area grid map [E*N][dagm_height][dagm_width], NULL if unused     */
  uint8_t* dagm;
  /* collisions (smarts.py:1270-1291, sensors.py:206-211): bit j = the agent's chassis touches the vehicle in
   * slot j of its env this tick — one Collision(collidee_id) per set bit; events[SMX_EV_COLLISIONS] = any bit */
  uint64_t* collidees;   /* [E*N]                                             */
  /* road waypoints (RoadWaypoints.lanes, sensors.py:999-1012), NULL if unused; L = rw_lanes, P = rw_paths,
   * R = 2 * rw_horizon + 1.  Rows beyond a count are not written. */
  uint8_t* rw_lane_count;   /* [E*N]          lanes the sensor reports (may exceed L)              */
  int16_t* rw_lane;         /* [E*N][L]       their lane ids in the reference's dict order, -1 none */
  int16_t* rw_path_count;   /* [E*N][L]       paths of that lane (may exceed P; saturates at 32767)  */
  uint8_t* rw_count;        /* [E*N][L][P]    waypoints of the kept path (0 = no such path)         */
  double* rw_pos;           /* [E*N][L][P][R][3]                                                    */
  float* rw_heading;        /* [E*N][L][P][R]                                                       */
  float* rw_lane_width;
  float* rw_speed_limit;
  int8_t* rw_lane_index;
  int16_t* rw_lane_id;
  /* auto_reset only, all five or none (NULL): the low-dimensional rows of the FINISHING tick of an env that restarts
   * inside the launch — the observation the reference hands back as info[agent]["env_obs"]
   * (smarts/env/wrappers/parallel_env.py:303-309, smarts/env/hiway_env.py:243-246) — copied by k_commit before the
   * reset pass overwrites ego_pos / ego_f32 / ego_lane / events / dist with the next episode's first observation.  Written
   * only for the slots of an env whose env_done is raised this tick; same layouts as their namesakes. */
  double* final_ego_pos;
  float* final_ego_f32;
  int16_t* final_ego_lane;
  uint8_t* final_events;
  double* final_dist;
  /* SMX_SENSOR_LANE_TTC, NULL if unused: lane_ttc of every agent with an observation in this pass, written after
   * the waypoint, neighbour and ego rows it is a function of — speeds and headings are the float32 values of those
   * rows, positions float64, lane identity wp_lane_id / nb_lane_id (-1 never matches).  Rows of agents without an
   * observation keep their values and read flags 0.  Under auto_reset the row of a restarted env describes its
   * first observation; there is no final_* twin (the finishing tick's env_obs is low-dimensional). */
  double* lane_ttc;        /* [E*N][SMX_TTC_COUNT]                             */
  uint8_t* lane_ttc_flags; /* [E*N] SMX_TTC_* bits                             */
  /* SMX_SENSOR_EGO_CENTRIC, all NULL if unused, and a row NULL where its sensor is off: the pass's rows in the frame
   * F = (px, py, pz, H) of the agent's own vehicle — (px, py, pz) its ego_pos row, H the float64 heading that
   * ego_f32[SMX_EGO_HEADING] is the rounding of.  With c = cos(-H), s = sin(-H) (_gen_ego_frame_matrix, math.py:464-470):
   *   to_ego(p) = (c dx - s dy, s dx + c dy, dz), d = p - (px, py, pz)        (position_to_ego_frame, math.py:473-487)
   *   rel(h)    = Heading(wrap_value(h - H, -pi, pi))                          (math.py:452-461, coordinates.py:175-184)
   *   dyn(v)    = (|v[:2]|, 0, v[2])                                           (ego_frame_dynamics, adapter :66-67)
   * float32 inputs are widened to float64, transformed and rounded back; positions stay float64.  Entries beyond
   * wp_count / nb_count / the rw_* counts are neither read nor written.  Rows of agents without an observation in the
   * pass keep their contents and read ec_flags 0.  Under auto_reset the rows of a restarted env describe its first
   * observation; there is no final_* twin.  Everything frame-independent (widths, speed limits, lane ids, counts,
   * grids) is read from the world rows. */
  double* ego_frame;      /* [E*N][4] px, py, pz, H: the frame itself (the adapters' last_obs)              */
  uint8_t* ec_flags;      /* [E*N] bit 0: the agent had an observation in this pass, its rows were written  */
  float* ec_ego_f32;      /* [E*N][SMX_EGO_F32_COUNT] heading 0, dyn() on linear velocity / acceleration / jerk, the rest copied */
  double* ec_wp_pos;      /* [E*N][wp_paths][wp_len][3] to_ego(), z = 0                                     */
  float* ec_wp_heading;   /* [E*N][wp_paths][wp_len] rel()                                                  */
  double* ec_nb_pos;      /* [E*N][nb_max][3]                                                               */
  float* ec_nb_heading;   /* [E*N][nb_max]                                                                  */
  double* ec_lidar_point; /* [E*N][lidar_rays][3]; a ray with lidar_hit 0 reads three NaNs (the reference's 0 * inf) */
  double* ec_rw_pos;      /* layout of rw_pos                                                               */
  float* ec_rw_heading;   /* layout of rw_heading                                                           */
  /* what the caller allocated: element count and SMX_DT_* of each buffer above, in declaration order
   * (SMX_OUT_*); 0 / SMX_DT_NONE for a NULL pointer */
  uint64_t count[SMX_OUT_BUFFERS];
  uint8_t dtype[(SMX_OUT_BUFFERS + 7) & ~7]; /* (rounded up: keeps the struct a multiple of 8 bytes) */
} smx_outputs;

/* ---- entry points ---- */
/* On failure no handle is left behind (*out = NULL); smx_last_error(NULL) then gives the reason. */
int smx_create(const smx_config* cfg, int device, smx_handle* out);
/* The entry check of smx_reset / smx_step*, callable on its own and without a device: every buffer the
 * configuration needs is non-NULL, declared with the expected SMX_DT_* and at least as many elements as
 * the configuration implies (a short buffer would be an out-of-bounds device write).  `has_vias`: vias
 * were given (smx_set_vias).  Returns SMX_OK or SMX_ERR_INVALID with the reason in err[err_len]. */
int smx_check_buffers(const smx_config* cfg, int has_vias, const smx_state* st, const smx_spawns* sp,
                      const smx_outputs* out, char* err, uint64_t err_len);
int smx_load_map(smx_handle h, const smx_map_tables* map);
/* Via points of the agents' missions (plan.py:180-188; ViaSensor sensors.py:1090-1149).  One list per
 * agent slot, shared by every env: vias[slot_off[s] .. slot_off[s+1]) belong to slot s (at most 32
 * each).  Host pointers; the library keeps a device copy.  n = 0 clears. */
typedef struct smx_via {
  double x, y;            /* Via.position */
  double hit_distance;
  double required_speed;
  int32_t lane;           /* Via.lane_id as a lane table index */
  int32_t pad;
} smx_via;
int smx_set_vias(smx_handle h, const smx_via* vias_host, int32_t n, const int32_t* slot_off_host);
/* Missions of the agent slots (plan.py:196-222, 316-349), shared by every env like the vias: n_slots = 0
 * clears, else n_slots = cfg.num_vehicles.  route_len = 0: endless mission with an empty route (plan.py:321-323,
 * what every slot has until this is called).  Otherwise a fixed route: roads[route_off .. route_off + route_len)
 * are road table indices in route order (RoadMap.Route.roads as sumo_road_network.py:711-765 generates them:
 * junction-internal roads included) and the goal is a PositionalGoal (plan.py:86-120).  With a fixed route
 * the waypoint paths of the controller and the waypoints sensor follow the route (sumo_road_network.py:822-829,
 * 862-882; lanepoints.py:666-683), off_route / reached_goal are live (sensors.py:491-496, 527-578) and the trip
 * meter counts only waypoints on the route (sensors.py:908-913).  Host pointers; the library keeps a device
 * copy.  Waits for the device; not to be called between smx_step and the use of its outputs. */
typedef struct smx_mission {
  double goal_x, goal_y, goal_radius;
  int32_t route_off, route_len;
} smx_mission;
int smx_set_missions(smx_handle h, const smx_mission* missions_host, int32_t n_slots, const int32_t* route_roads_host,
                     int32_t n_route_roads);
/* Goal kinds of the agent slots beyond the PositionalGoal of smx_set_missions.  A call of its own, after
 * smx_set_missions (which leaves every slot SMX_GOAL_POSITIONAL): n_slots = 0 clears, else n_slots = cfg.num_vehicles.
 *  - SMX_GOAL_POSITIONAL: what smx_set_missions set (num_laps and route_length are not read).
 *  - SMX_GOAL_LAP (plan.py:252-277, LapMission.is_complete): the slot has a fixed route and a PositionalGoal from
 *    smx_set_missions; reached_goal = inside the goal radius AND distance_travelled > route_length * num_laps, the
 *    trip meter's total after this tick's waypoint (sensors.py:491-496).  num_laps >= 1, route_length finite, >= 0.
 *  - SMX_GOAL_TRAVERSE (plan.py:127-166, TraverseGoal._drove_off_map): the slot has an empty route
 *    (smx_mission.route_len = 0); reached_goal = the vehicle has left the map beyond the end of a dead-end lane,
 *    heading within pi/6 of the lane's end heading.  Needs the two per-lane facts below.
 * lane_end_heading[n_lanes] (vec_to_radians of the lane's vector_at_offset(length - 0.1), from the host's libm) and
 * lane_dead_end[n_lanes] (1: no outgoing lanes, via lanes counted as outgoing; sumo_road_network.py:351-358) are
 * read only when some slot is SMX_GOAL_TRAVERSE (else they may be NULL, n_lanes 0); n_lanes = the map's.  Host
 * pointers; the handle keeps a device copy (12 bytes a lane), dropped by smx_set_missions and smx_load_map.
 * smx_check_mission_goals is the validation alone, callable without a device or a handle (map_lanes: the lane
 * count of the map the table is for): SMX_OK, or SMX_ERR_INVALID with the reason in err[err_len]. */
enum { SMX_GOAL_POSITIONAL = 0, SMX_GOAL_LAP = 1, SMX_GOAL_TRAVERSE = 2 };
typedef struct smx_mission_goal {
  int32_t kind;         /* SMX_GOAL_* */
  int32_t num_laps;     /* SMX_GOAL_LAP */
  double route_length;  /* SMX_GOAL_LAP: Route.road_length of the lap (scenario.py:715-746) */
} smx_mission_goal;
int smx_check_mission_goals(const smx_mission_goal* goals_host, int32_t n_slots, int32_t num_vehicles,
                            const double* lane_end_heading_host, const int32_t* lane_dead_end_host, int32_t n_lanes,
                            int32_t map_lanes, char* err, uint64_t err_len);
int smx_set_mission_goals(smx_handle h, const smx_mission_goal* goals_host, int32_t n_slots,
                          const double* lane_end_heading_host, const int32_t* lane_dead_end_host, int32_t n_lanes);
/* A mission pool: missions per env and per episode, off unless bound (scenario.py:206-227, 292-294: a scenario's missions
 * are handed out as variations, one after another, and every ParallelEnv worker runs its own cycle).  The pool is
 * n_missions <= SMX_MISSION_POOL_MAX missions, each with what one slot has through the three calls above:
 *   missions_host [n_missions] and route_roads_host [n_route_roads], as for smx_set_missions;
 *   goals_host    [n_missions] as for smx_set_mission_goals, or NULL: every goal positional; the two lane tables and
 *                 n_lanes as there (read only when some goal is SMX_GOAL_TRAVERSE);
 *   vias_host     [n_vias] and via_off_host [n_missions + 1]: vias[via_off[m] .. via_off[m+1]) belong to mission m, at
 *                 most 32 each; n_vias = 0: none (both may be NULL).  Needs cfg.via_max > 0 when n_vias > 0.
 * Host pointers; the library keeps device copies.  The checks are those of the three calls, per pool entry.
 *   rows_dev      int32 [rows][E][A] (A = num_vehicles - num_social), DEVICE memory owned by the caller, rows_count = the
 *                 elements allocated (>= rows * E * A).  Agent a of env e has mission rows_dev[k mod rows][e][a] in
 *                 episode k (the episode counter of smx_state::env_episode, as for smx_agent_dims).  -1 = an endless
 *                 mission with an empty route and no vias, what a slot has before smx_set_missions.  Social slots have no
 *                 entry and no mission.
 * The library cannot check a device table, so the device is safe on its own: an entry outside -1 .. n_missions - 1 is
 * read as -1, never indexes a table, and makes the next smx_sync return SMX_ERR_INVALID (once; the bit is cleared).
 * The table is read by EVERY pass, wherever a mission is needed: rewriting the row of a running episode changes that
 * agent's route, goal and vias in the middle of the episode (its via hits so far are kept by position in the list);
 * rows of episodes not yet started may be rewritten freely — a curriculum sampled on the device.  The finishing tick of
 * an episode reads the old episode's row; the reset pass, a restart inside the launch under auto_reset included, the
 * new one's.
 * The pool and the per-slot tables exclude each other: binding a pool drops what smx_set_missions /
 * smx_set_mission_goals / smx_set_vias bound, and while a pool is bound those three return SMX_ERR_STATE.  pool = NULL
 * unbinds: every mission is endless again, with no vias.  smx_load_map drops the pool as it drops the missions.  Waits
 * for the device; not to be called between smx_step and the use of its outputs.
 * smx_check_mission_pool is the validation alone, callable without a device or a handle (`map`: the tables of the map
 * the pool is for; rows_dev is only tested for NULL): SMX_OK, or SMX_ERR_INVALID with the reason in err[err_len]. */
#define SMX_MISSION_POOL_MAX 4096
typedef struct smx_mission_pool {
  const smx_mission* missions_host;
  const int32_t* route_roads_host;
  const smx_mission_goal* goals_host;
  const double* lane_end_heading_host;
  const int32_t* lane_dead_end_host;
  const smx_via* vias_host;
  const int32_t* via_off_host;
  const int32_t* rows_dev;
  uint64_t rows_count;
  int32_t n_missions, n_route_roads, n_lanes, n_vias, rows, pad;
} smx_mission_pool;
int smx_set_mission_pool(smx_handle h, const smx_mission_pool* pool);
int smx_check_mission_pool(const smx_config* cfg, const smx_map_tables* map, const smx_mission_pool* pool, char* err,
                           uint64_t err_len);
/* Base ray directions (device, [lidar_rays][3]); reference lidar.py:89-113 */
int smx_set_lidar_rays(smx_handle h, const double* rays_dev, int32_t n_rays);
/* The image buffer of SMX_SENSOR_RGB (device, caller-owned, [E*N][rgb_height][rgb_width][3] uint8; `count` = the bytes
 * allocated; 16-byte aligned: the image is written with 16-byte stores).  It may be called again between ticks to alternate buffers; NULL unbinds.  A buffer shorter than the
 * configuration implies is SMX_ERR_INVALID (it would be an out-of-bounds device write); smx_reset / smx_step* with the
 * sensor on and no buffer bound return SMX_ERR_STATE.  smx_check_rgb_output is the validation alone, callable without a
 * device or a handle: the bit against the grid, the grid limits, and `count` against E * N * rgb_height * rgb_width * 3
 * (with the bit off any count passes).  SMX_OK, or SMX_ERR_INVALID with the reason in err[err_len]. */
int smx_set_rgb_output(smx_handle h, uint8_t* rgb_dev, uint64_t count);
int smx_check_rgb_output(const smx_config* cfg, uint64_t count, char* err, uint64_t err_len);
/* The state guard, off by default.  State rows, spawn tables and action buffers are the caller's; while a guard buffer
 * is bound, no alive agent vehicle's pose reaches a map search, a sensor or another vehicle's sensor unless it is IN
 * BOUNDS: the seven words x, y, heading, u, v, r, delta of its state finite (a kinematic agent: x, y, heading, u; a
 * spawn row: its four words) and (x, y) inside the guard box — the union of the extents of the map's lanepoint grid
 * (lpg_*) and segment grid (sg_*), grown by `margin` metres on every side.  The offending agent's episode ends instead
 * (the reference destroys the simulation and asks for a reset, smarts.py:214-227, 1014-1046):
 *   - every smx_reset / smx_step* pass writes guard_dev[e * N + slot] for every slot: 0 for a social slot, an agent
 *     absent from the pass and an agent in bounds, else the bits below;
 *   - SMX_GUARD_STEP: all state rows 0 .. SMX_S_MCL_Y and the flags word keep their values from the start of the tick
 *     (the flags word gains SMX_F_GUARDED); the kinematic spaces' "not finite -> no action" (smx_sync) is unchanged;
 *   - SMX_GUARD_STATE: neither controller nor dynamics run; the vehicle is parked — the pose of lanepoint 0
 *     (lp_rec[0], always on the map), velocities, yaw rate and steer 0, the controller state as after a reset;
 *   - SMX_GUARD_SPAWN: the vehicle is created parked; the bit is reported by the reset pass and again by the first
 *     step, whose observation ends the agent (reset passes report no done);
 *   - the agent's observation is built from the held or parked pose like any other (`events` is whatever that pose
 *     yields; no tenth event column), with done = 1 and active = 0; it counts in env_done_count, its vehicle is removed
 *     like any done agent's, and under auto_reset the env restarts as usual.
 * The same launches run either way; with the guard off the kernels are the ones without it (a compile-time choice).
 * Out of scope: social slots (the library derives their pose from its own tables), the controller-state rows as such
 * (a NaN there surfaces as SMX_GUARD_STEP one tick later) and what smx_sync reports (unchanged).
 * `margin`: finite, 0 <= margin <= SMX_GUARD_MARGIN_MAX.  The cap keeps the cell index of every in-bounds point inside
 * int32 with room to spare and bounds every ring loop of the searches: |index| <= (2.5 side + 1024) / cell + 1, `side`
 * the longer side of the grown box and `cell` the smaller of the two grids' cells, must stay below 2^30 — checked
 * against the map here, and by smx_load_map when the guard is bound first (which also recomputes the box for a new map
 * and keeps the guard bound).  At 1.0e6 m and cells of a metre or more that leaves room for a map 4.2e8 m across; the
 * derivation is in smarts_amd/csrc/smx_guard.h.  guard_dev = NULL switches the guard off.  smx_check_guard is the
 * validation alone (count >= E * N, the margin), callable without a device or a handle: SMX_OK, or SMX_ERR_INVALID
 * with the reason in err[err_len]. */
enum { SMX_GUARD_STEP = 1 << 0,   /* this tick's step produced an out-of-bounds state: not stored, the vehicle is held */
       SMX_GUARD_STATE = 1 << 1,  /* the state at the start of the tick was out of bounds already (the caller wrote it) */
       SMX_GUARD_SPAWN = 1 << 2   /* the spawn row of this episode was out of bounds */ };
#define SMX_GUARD_MARGIN_DEFAULT 1000.0
#define SMX_GUARD_MARGIN_MAX 1.0e6
int smx_set_guard(smx_handle h, uint8_t* guard_dev, uint64_t count, double margin);   /* [E*N]; NULL = guard off */
int smx_check_guard(const smx_config* cfg, uint64_t count, double margin, char* err, uint64_t err_len);
/* Traffic-history replay (TrafficHistoryProvider, smarts/core/traffic_history_provider.py:94-170 over
 * traffic_history.py): while a history is bound, the social slots (the last cfg.num_social of every env) take pose,
 * speed and presence from a recorded table instead of the scripted lane follower; without one nothing changes.
 *   frames_host[n_frames][num_social][4]  x, y, heading, speed of the vehicle CENTRE, heading in the reference's
 *                                         convention and already wrapped as Heading.__new__ wraps it: the device copies
 *                                         the four words bit for bit into SMX_S_X / _Y / _HEADING / _U
 *   vehicle_host[n_frames][num_social]    the history's vehicle id in that slot and frame, < 0 = the slot is empty
 * Host pointers; the handle keeps a device copy (dropped by smx_load_map: the rows were checked against that map).  The
 * two device tables stay the caller's and are read in every pass, so rewriting them in place takes effect with the next
 * tick; any value in them is safe.
 *   frame  = (int64) start_frame[episode mod rows][env] + env_ticks, env_ticks the tick count the pass's observation
 *            reports (cfg.reset_elapsed_steps at a reset observation); outside [0, n_frames) every slot is empty
 *   present = vehicle[frame][slot] >= 0 and != replaced[episode mod rows][env]   (replaced_dev NULL: nothing hidden)
 * A present slot is an alive social vehicle at the frame's row: seen by every sensor and collision test, with the
 * sedan's box (or its own: smx_set_social_history_dims below).  SMX_S_PREV_X / _Y behave as for the scripted vehicle, SMX_S_MCL_X / _Y / SMX_S_SPD_INT stay 0;
 * spawns.social and the slot's spawns.pose rows are not read (the entry check still wants the buffer).  An absent slot
 * is not alive; it never counts in env_done_count or env_done.  SMX_F_ALIVE of a social slot is decided at the end of
 * the pass before (from the tables as they were then): after an in-place rewrite a vehicle that the new frame lacks
 * leaves at once, one that it adds enters a tick late.
 * Refused (SMX_ERR_INVALID, the reason in smx_last_error): num_social different from the configuration's or 0;
 * n_frames < 1 or sizes that overflow; cfg.social_model == SMX_SOCIAL_IDM (the replay replaces the speed model);
 * start_count / replaced_count below rows * num_envs; rows < 1; a row of a non-empty slot that is not finite or lies
 * outside the union of the map's two grids (smx_set_guard's box with margin 0: the state guard does not cover social
 * slots, this check does).  Needs the map (SMX_ERR_STATE before smx_load_map).  hist = NULL unbinds.  Waits for the
 * device.  smx_check_social_history is the validation alone, callable without a device or a handle (`map`: only the
 * grid extents lpg_* / sg_* are read). */
typedef struct smx_social_history {
  const double* frames_host;   /* [n_frames][num_social][4] */
  const int32_t* vehicle_host; /* [n_frames][num_social], < 0 = empty */
  int32_t n_frames, num_social;
  const int32_t* start_frame_dev; /* device, caller-owned, [rows][num_envs]; read every tick */
  const int32_t* replaced_dev;    /* device, caller-owned, [rows][num_envs] vehicle id hidden in that env; -1 none; may be NULL */
  int32_t rows;
  uint64_t start_count, replaced_count; /* int32 elements the caller allocated for each */
} smx_social_history;
int smx_set_social_history(smx_handle h, const smx_social_history* hist);
int smx_check_social_history(const smx_config* cfg, const smx_map_tables* map, const smx_social_history* hist, char* err,
                             uint64_t err_len);
/* ... at each vehicle's own dimensions (TrafficHistoryProvider.step, traffic_history_provider.py:112-126).  Opt-in: with
 * a history bound and no dimensions every replayed vehicle has the sedan's box, as before.
 *   dims_host[n_ids][3]   length, width, height in metres of the history's vehicle `id`, the provider's rule already
 *                         applied (the dataset's value, or the default of the vehicle's type where it has none)
 * A host pointer; the handle keeps a device copy and a triple per (env, slot).  The triple is written wherever the
 * replayed slot's pose is written, looked up through the frame's vehicle id: the size a pass's sensors see is that of
 * the vehicle whose pose they see, a slot reused by another vehicle changes size with it, and an in-place rewrite of
 * start_frame / replaced takes effect together with the pose.  Read by: the collision test (two sizes; the broad phase
 * reaches the sedan's half diagonal plus the mate's plus the leeway), nb_box (cast to float32), the OGM, the RGB image
 * and the lidar (the mate's half length and half width; vertically the box keeps the sedan's underside,
 * SMX_BASE_HEIGHT + 0.1, and rises by the vehicle's height — the reference centres a BoxChassis box on z = 0, this path
 * stands every vehicle on the ground).  Not read by: the state rows of replayed slots (unchanged), the scripted models,
 * and anything of an agent's own box: its ego box row, its off-route and path-seed radii, its neighbours' lane lookup (the
 * EGO's length, sensors.py:244-246) are the agent's (smx_set_agent_dims below; without it agents are sedans, an agent
 * that stands in for a recorded truck, `replaced`, included).
 * Needs a bound history (SMX_ERR_STATE without one); smx_set_social_history, with a table or NULL, and smx_load_map
 * drop the dimensions.  dims = NULL unbinds: the sedan's box again from the next tick.  Refused (SMX_ERR_INVALID, the
 * reason in smx_last_error): n_ids < 1; a non-empty cell of the bound vehicle_host whose id is >= n_ids; a value that is
 * not finite or <= 0; length or width above 25 m; height above 10 m.  Waits for the device.
 * smx_check_social_history_dims is the validation alone, without a device or a handle (`hist`: vehicle_host, n_frames
 * and num_social are read). */
typedef struct smx_social_dims {
  const double* dims_host; /* [n_ids][3] length, width, height */
  int32_t n_ids;
} smx_social_dims;
int smx_set_social_history_dims(smx_handle h, const smx_social_dims* dims);
int smx_check_social_history_dims(const smx_config* cfg, const smx_social_history* hist, const smx_social_dims* dims, char* err,
                                  uint64_t err_len);
/* Per-agent vehicle dimensions (Vehicle.agent_vehicle_dims -> BoxChassis, vehicle.py:339-357, 426-431; a recorded
 * vehicle keeps its own when an agent takes it over, vehicle_index.py:439, 489).  Opt-in: with nothing bound every agent
 * has the sedan's box, as before.
 *   dims_host[rows][num_envs][num_agents][3]   length, width, height in metres (num_agents = num_vehicles - num_social);
 *                                              three NaNs = the sedan's box
 *   rows                                       an episode uses row (episode mod rows), as the spawn tables do
 * A host pointer; the handle keeps a device copy and a triple per (env, vehicle) — the block smx_set_social_history_dims
 * uses, which exists while either binding holds.  An agent's triple is written where its spawn pose is (a reset, the
 * restart inside a launch under auto_reset, a history agent's placement) and nowhere else: a follower that is later
 * shadowed, handed over, hijacked or released keeps it.  Read by everything that asks for a box: the agent's own
 * collision test, the four corners behind on_shoulder / off_road, its ego box row, the lane lookups within its length
 * (its neighbours' lane ids, the trip meter's first waypoint), its off_route radius (half diagonal + 5), and, as an
 * env-mate, nb_box, the OGM, the RGB image and the lidar.  Not read by: motion (the kinematic spaces move a pose), the
 * scripted models' gap, lane-TTC, road waypoints, bubbles and the state guard.
 * The kinematic spaces only (SMX_ACTION_SPACE_TARGET_POSE, _TRAJECTORY_WITH_TIME, _IMITATION — and so every history
 * agent): the dynamic spaces' model constants are the sedan's.  Deviation: the reference ignores the dimensions of an
 * agent on a dynamic chassis with a warning (vehicle.py:410-415); here the call is refused.
 * The cap.  Length <= 10 m, width <= 25 m, height <= 10 m (the reference's largest type, the trailer, is 10 x 2.5 x 4).
 *   length  An observer reports a neighbour's lane as nearest_lane(neighbour, radius = the OBSERVER's length)
 *           (sensors.py:245).  That lookup is answered from the neighbour's own road-facts search, which — for a social
 *           slot and for an agent alike — runs at SMX_POSE_SCAN_RADIUS = 10 m (or two lane widths where that is more)
 *           and keeps a lane only at a distance below that radius.  An observer longer than 10 m would be told "no lane"
 *           for a neighbour whose lane is 10 m or more away where the reference finds one, so the length is capped at
 *           that radius (SMX_AGENT_DIMS_MAX_LENGTH; the trailer's 10 m is exact: "dist < 10" is "dist < length").  A
 *           recorded vehicle longer than 10 m can be replayed (smx_set_social_history_dims) but not followed at its
 *           own length.
 *   width   The agent's OWN lookups need a search that follows its box, and get one on this path: it runs at
 *           radius = max(SMX_POSE_SCAN_RADIUS, half diagonal + max(5, widest road_with_point threshold)) — the
 *           off_route radius is half diagonal + 5, 10.15 m for the trailer — and keeps every segment within threshold
 *           + half diagonal of the centre, which covers the four corners (the sedan: the 10 m and 2 m of the path
 *           without dimensions); the collision test's broad phase is boxes_within's own (half diagonal + the mate's +
 *           the leeway).  Neither bounds the width; what does is what bounds a replayed vehicle's: the reaches and
 *           pixel rectangles the mate-side consumers form from a triple, SMX_DIMS_MAX_PLANAR = 25 m.
 *   height  SMX_DIMS_MAX_HEIGHT = 10 m, as for a replayed vehicle (the lidar's box).
 * A box that outgrows the one-lane scan's candidate lists (SMX_FACTS_SPAN grid rows: a trailer's reach often does) is
 * served by the team form through the slow list, as any vehicle those cannot serve.
 * Refused (SMX_ERR_INVALID, the reason in smx_last_error): another action space; a null table; rows < 1; a component that
 * is not finite, <= 0 or above its cap; a triple that is only partly NaN.  dims = NULL unbinds: every agent is a sedan
 * again from its next (re)spawn (at once when no social dimensions are bound either).  smx_set_social_history, with a
 * table or NULL, keeps the agents' dimensions (it drops the social ones); smx_load_map drops both.  Waits for the device.
 * smx_check_agent_dims is the validation alone, without a device or a handle. */
typedef struct smx_agent_dims {
  const double* dims_host; /* [rows][num_envs][num_agents][3] length, width, height; NaN x 3 = the sedan's */
  int32_t rows;
} smx_agent_dims;
int smx_set_agent_dims(smx_handle h, const smx_agent_dims* dims);
int smx_check_agent_dims(const smx_config* cfg, const smx_agent_dims* dims, char* err, uint64_t err_len);
/* History agents (the reference's SMARTS.attach_sensors_to_vehicles + observe_from over a traffic history, smarts.py:
 * 914-921: a recorded vehicle that carries sensors is a BoxChassis moved by Vehicle.control(pose, speed, dt)).  While
 * bound, agent slot `a` of env `e` follows recorded vehicle
 *   v = vehicle_dev[episode mod rows][e][a]      (rows = the bound history's; A = num_vehicles - num_social agents an env)
 * of the bound history; v < 0 = the slot follows nothing.  `frame` as for the social slots (smx_social_history).
 *   hidden twin  a social slot whose id equals any v >= 0 of its env's agents is absent (beside `replaced`), in every
 *                pass and through every entry point, whatever became of the follower.
 *   reset        a follower's spawn is v's row of the reset observation's frame — x, y, heading, speed word for word,
 *                SMX_S_KIN_RAW_HEADING that heading, SMX_S_KIN_LAST_DT 0 — instead of spawns.pose (still wanted by the
 *                entry check).  With v < 0, or v not in that frame, the agent does not enter: not alive, its rows an
 *                absent agent's, status SMX_HA_ABSENT, and the env's done count starts at the number of such agents (an
 *                env with no agent present is done after its first tick).
 *   step         smx_step_history_agents is a tick in which no agent sends an action: a follower whose vehicle is in
 *                the frame of the coming observation is placed on its row (SMX_S_PREV_X / _Y as in every tick,
 *                SMX_S_KIN_LAST_HEADING the heading held, SMX_S_KIN_LAST_DT dt, then the four words, no wrap: the table
 *                is wrapped).  One whose vehicle the frame lacks LEAVES: nothing of its state is stored, the tick's
 *                observation is built from the held pose with done = 1, active = 0, status SMX_HA_LEFT, and it counts as
 *                a finished agent (SMX_F_LEFT, applied by the tick's commit).  It does not come back.  The state guard,
 *                if on, tests the held state as in every tick; the byte of a follower reads 0 (the table was checked
 *                against the grids when it was bound).
 *   action_dev   (optional) [E*N][3] float32 in smx_step_continuous' Imitation layout, written wherever a follower's
 *                pose is written (the reset pass, every following tick): the inverse of ImitationController between
 *                frame f and f + 1, acceleration = (speed[f+1] - speed[f]) / dt, angular_velocity =
 *                min_angles_difference_signed(heading[f+1], heading[f]) / dt, in float64, rounded once, third word 0;
 *                NaN, NaN, 0 where the vehicle is not in f + 1 and for absent / left agents.  Social rows never written.
 *   status_dev   (optional) [E*N] SMX_HA_*, agents' bytes only.
 * smx_step_continuous keeps working on a bound sim: that tick drives every agent by its Imitation action from the
 * recorded state it holds, the twins stay hidden, action_dev / status_dev are not written; a following tick afterwards
 * puts the vehicles back on the recording.  Agents stay sedans.
 * Needs cfg.action_space == SMX_ACTION_SPACE_IMITATION (SMX_ERR_INVALID otherwise) and a bound history (SMX_ERR_STATE
 * without one); refused (SMX_ERR_INVALID): vehicle_dev NULL, vehicle_count < rows * num_envs * A, action_count < 3 * E * N
 * or status_count < E * N for a pointer that is given, no agent slot.  Any value in vehicle_dev is safe: ids are only
 * compared.  ha = NULL unbinds; smx_set_social_history (table or NULL) and smx_load_map drop the binding.  Waits for the
 * device.  smx_check_history_agents is the validation alone, without a device or a handle (`hist`: rows is read).
 * smx_step_history_agents without a binding: SMX_ERR_STATE. */
typedef struct smx_history_agents {
  const int32_t* vehicle_dev; /* device, caller-owned, [rows][num_envs][A] followed vehicle id, < 0 = none; read every pass */
  uint64_t vehicle_count;     /* int32 elements allocated */
  float* action_dev;          /* device, caller-owned, [E*N][3] expert action; may be NULL */
  uint8_t* status_dev;        /* device, caller-owned, [E*N]; may be NULL */
  uint64_t action_count, status_count;
} smx_history_agents;
enum { SMX_HA_FOLLOWING = 0, SMX_HA_LEFT = 1, SMX_HA_ABSENT = 2 };
int smx_set_history_agents(smx_handle h, const smx_history_agents* ha);
int smx_check_history_agents(const smx_config* cfg, const smx_social_history* hist, const smx_history_agents* ha, char* err,
                             uint64_t err_len);
/* Handing history agents over to actions one by one, inside a tick (the reference's SMARTS.add_agent_and_switch_control /
 * switch_control_to_agent, smarts.py:505-561, vehicle_index.py:392-457, and a bubble over a replayed history,
 * bubble_manager.py:208-218: one recorded vehicle leaves the TrafficHistoryProvider and is a BoxChassis at the pose and
 * speed it holds, moved by its agent's action while every other recorded vehicle keeps replaying).  A handover table
 * beside the follow table, and a tick that reads both: with
 *   H = tick_dev[episode mod rows][e][a]          (indexed exactly as vehicle_dev is)
 *   driven       in an smx_step_history_handover tick that starts with env_ticks[e] = t, agent `a` is DRIVEN iff
 *                H >= 0 && t >= H; otherwise it FOLLOWS.  The rule is stateless: the table is read every tick, so a
 *                caller may rewrite it in place; any value is safe (it is only compared); H = 0 drives from the first
 *                tick after the reset, H < 0 never drives.
 *   a follower   does, word for word, what smx_step_history_agents does with it: placed on its vehicle's row of the
 *                coming frame with SMX_S_KIN_LAST_HEADING / _LAST_DT, or it leaves (SMX_F_LEFT, SMX_HA_LEFT); its
 *                expert action, status SMX_HA_FOLLOWING, a guard byte of 0.
 *   a driven one does, word for word, what smx_step_continuous does with an Imitation agent, from the state it holds and
 *                its row of actions_dev: a NaN first word = no control() call, a NaN second word = the scalar form;
 *                under the guard it gets the placement test.  Its status byte is SMX_HA_DRIVEN, its action_dev row
 *                NaN, NaN, 0.  It never sets SMX_F_LEFT: a driven agent whose recorded vehicle ends keeps driving.  Its
 *                recorded twin stays hidden from the social slots (the hidden-twin rule above).
 *   back         a driven agent that the table later turns into a follower again is put back on the recording, or
 *                leaves if the frame lacks its vehicle: what a following tick after smx_step_continuous does.
 *   not alive    SMX_HA_ABSENT and SMX_HA_LEFT agents are not alive: their H is ignored.
 *   reset        the reset pass (under auto_reset, inside the tick) is unchanged: the spawn comes from the recording, the
 *                status is FOLLOWING / ABSENT, the expert action is written; the next tick reads the new episode's row.
 * smx_step_history_agents and smx_step_continuous behave on a sim with a handover bound exactly as without: the table is
 * ignored.  Followers' and social rows of actions_dev are never read.
 * smx_set_history_handover needs bound history agents (SMX_ERR_STATE otherwise); refused (SMX_ERR_INVALID): tick_dev NULL,
 * tick_count < rows * num_envs * A.  ho = NULL unbinds; smx_set_history_agents (table or NULL), smx_set_social_history
 * and smx_load_map drop the binding.  Waits for the device.  smx_check_history_handover is the validation alone, without
 * a device or a handle (`hist`: rows is read).  smx_step_history_handover without a binding: SMX_ERR_STATE; with
 * actions_dev == NULL: SMX_ERR_INVALID. */
typedef struct smx_history_handover {
  const int32_t* tick_dev; /* device, caller-owned, [rows][num_envs][A]; read every pass */
  uint64_t tick_count;     /* int32 elements allocated */
} smx_history_handover;
enum { SMX_HA_DRIVEN = 3 }; /* a history agent driven by its action in this tick (smx_step_history_handover) */
int smx_set_history_handover(smx_handle h, const smx_history_handover* ho);
int smx_check_history_handover(const smx_config* cfg, const smx_social_history* hist, const smx_history_handover* ho, char* err,
                               uint64_t err_len);
/* Bubbles over a replayed history, evaluated on the device (the reference's BubbleManager.step, bubble_manager.py:393-463,
 * for PositionalZone bubbles; DESIGN.md section 5.21 restates the rule).  While bound, every smx_step_history_handover tick
 * starts with a bubble pass over the poses the previous pass left; it keeps one state byte and one cursor byte per agent:
 *   state_dev    [E*N] SMX_BUBBLE_SOCIAL / _SHADOWED / _HIJACKED / _RELEASED, agents' bytes only, valid for the episode
 *   cursor_dev   [E*N] bit b set: the agent's cursor at bubble b had a state (InBubble / InAirlock) in the last pass
 * Both rows read 0 for an env after its reset pass (smx_reset, or under auto_reset inside the tick).
 *   geometry     a bubble is the rectangle size_x x size_y (inner zone) and the same rectangle grown by `margin` on every
 *                side (airlock); boundaries are outside.  follow_agent < 0: centred at (x, y), axis-aligned.
 *                follow_agent = k: pinned to agent slot k of the same env, q = R(-heading_k) (p - p_k) - (offset_x,
 *                offset_y), (x, y) unused; inactive (no cursors, its cursor bits clear, states stay) while k is not alive.
 *   the pass     agents in ascending slot, bubbles in ascending index; only alive agents have cursors; limits count the
 *                agents the previous pass left hijacked / shadowed at the bubble and the cursors made earlier in this pass
 *                (0 = no limit).  SOCIAL -> SHADOWED in the airlock, SHADOWED -> HIJACKED inside, HIJACKED -> RELEASED and
 *                SHADOWED -> SOCIAL once outside both.  An agent the handover table drives in the tick makes no transition.
 *   the tick     an agent is DRIVEN iff the handover table says so (when one is bound) or its state is HIJACKED: status
 *                SMX_HA_DRIVEN, as a table-driven agent in every word.  SOCIAL and SHADOWED agents follow as in every
 *                mixed tick, status SMX_HA_FOLLOWING / SMX_HA_SHADOWED, expert action written for both.  A RELEASED agent
 *                ends as a leaving follower ends: nothing stored, observed once more at the held pose with done = 1,
 *                active = 0, counted as finished (SMX_F_LEFT), status SMX_HA_RELEASED; its recorded twin stays hidden.
 * smx_step_history_agents and smx_step_continuous ignore the bubbles and do not touch the two rows.
 * smx_set_history_bubbles needs bound history agents (SMX_ERR_STATE otherwise); refused (SMX_ERR_INVALID): n_bubbles
 * outside 1..SMX_MAX_BUBBLES, a field that is not finite, a size or margin <= 0, follow_agent >= A, a negative limit,
 * shadow_limit != 0 and < hijack_limit, a NULL row or one of fewer than E * N bytes.  hb = NULL unbinds; whatever drops
 * the history agents drops the bubbles.  With bubbles bound smx_step_history_handover needs no handover table.  Waits for
 * the device.  smx_check_history_bubbles is the validation alone, without a device or a handle. */
#define SMX_MAX_BUBBLES 8
typedef struct smx_bubble {
  double x, y, size_x, size_y, margin, offset_x, offset_y;
  int32_t follow_agent; /* agent slot of the same env the bubble travels with, -1 = fixed at (x, y) */
  int32_t hijack_limit, shadow_limit; /* 0 = none */
} smx_bubble;
typedef struct smx_history_bubbles {
  const smx_bubble* bubbles_host; /* host, [n_bubbles]; copied by the call */
  int32_t n_bubbles;
  uint8_t* state_dev;  /* device, caller-owned, [E*N] SMX_BUBBLE_* */
  uint8_t* cursor_dev; /* device, caller-owned, [E*N] one bit per bubble */
  uint64_t state_count, cursor_count;
} smx_history_bubbles;
enum { SMX_BUBBLE_SOCIAL = 0, SMX_BUBBLE_SHADOWED = 1, SMX_BUBBLE_HIJACKED = 2, SMX_BUBBLE_RELEASED = 3 };
enum { SMX_HA_SHADOWED = 4, SMX_HA_RELEASED = 5 }; /* following while shadowed by a bubble; released by one in this tick */
int smx_set_history_bubbles(smx_handle h, const smx_history_bubbles* hb);
int smx_check_history_bubbles(const smx_config* cfg, const smx_history_bubbles* hb, char* err, uint64_t err_len);
/* Delayed agent entry (the reference's Mission.start_time + TrapEntryTactic without a capture zone: trap_manager.py:53-65,
 * 121-241; DESIGN.md section 5.23 has the rule and its deviations).  Opt-in: with nothing bound every agent enters at the
 * reset observation, as before.  For agent `a` of env `e` in episode k (row = k mod rows):
 *   ready_host[row][e][a]     the tick, counted from the reset observation (tick 0), from which the agent may enter; >= 0,
 *                             and every (row, env) has an agent at 0 (the reset observation is the first that holds one)
 *   check_host[row][e][a][3]  x, y of the mission's start point (the front bumper, not the spawn centre) and the new
 *                             vehicle's largest plane dimension, in metres
 *   reset     an agent at tick 0 is created as before, with no overlap check.  Any other agent is PENDING: not alive, its
 *             rows an absent agent's (zeros, active = 0, done = 0), not counted in env_done_count — the env ends only
 *             when every agent has entered and become done, as in the reference.
 *   a tick    once the control phase has stepped every vehicle, a pending agent whose ready tick has come is BLOCKED in this
 *             tick when an alive social slot s of its env has dx*dx + dy*dy <= (0.5 * (max(l_s, w_s) + dim))^2, dx, dy
 *             the slot's position minus the check point (l_s, w_s: the slot's dimensions where smx_set_social_history_dims
 *             binds them, else the sedan's); agents are not checked.  Otherwise it ENTERS: created from its spawn row
 *             exactly as a reset creates it (pose, speed word, guard verdict, own dimensions), SMX_F_ALIVE | SMX_F_FIRST,
 *             before the observation pass.  Its observation in that tick is a first observation (steps 1, distance 0,
 *             no events carried) that runs its collision test (SMX_F_ENTERING); its action of that tick is not read; its env-mates see
 *             it in the same tick (neighbours, collisions, OGM, RGB, lidar).  A blocked agent tries again next tick.
 *   status_dev   [E*N] SMX_ENTRY_*, agents' bytes only: PENDING / BLOCKED until the agent enters, then ENTERED.
 *   entered_dev  [E*N] -1 until the agent enters, then the tick of its entry observation (counted from the reset
 *                observation: 0 for an agent that entered with it).
 * Every launch form: the small form's tick observes the entrant in its own pass; the large forms' tick, whose kernels
 * run over an alive list built a tick ahead, lets the mates see it (k_entry computes its road facts, so they report its
 * lane as the small form does) and gives it its first observation in the reset pass
 * after the commit (k_entry_first lists its env group), as a restart inside the tick does.
 * A bind or unbind (or a new map that drops the table) holds smx_step* (SMX_ERR_STATE) until an smx_reset of every env
 * (env_mask NULL): the status rows describe no episode before it, and a masked reset leaves envs that were not reset.
 * Refused (SMX_ERR_INVALID, the reason in smx_last_error): a null table or row, rows < 1, a negative tick, a (row, env)
 * with no agent at tick 0, a check row that is not finite or a dimension <= 0, status_count or entered_count < E * N;
 * SMX_ERR_STATE while history agents (and so handover or bubbles) or a frame stack are bound — and those are refused
 * while this is bound.  The tables are copied; the two rows are the caller's.  entry = NULL unbinds (every agent enters
 * at its next reset).  Waits for the device.  smx_check_agent_entry is the validation alone, without a device or a handle. */
typedef struct smx_agent_entry {
  const int32_t* ready_host; /* host, [rows][num_envs][A] ready tick; copied by the call */
  const double* check_host;  /* host, [rows][num_envs][A][3] x, y, largest plane dimension; copied by the call */
  int32_t rows;
  uint8_t* status_dev;  /* device, caller-owned, [E*N] SMX_ENTRY_* */
  int32_t* entered_dev; /* device, caller-owned, [E*N] */
  uint64_t status_count, entered_count;
} smx_agent_entry;
enum { SMX_ENTRY_PENDING = 0, SMX_ENTRY_BLOCKED = 1, SMX_ENTRY_ENTERED = 2 };
int smx_set_agent_entry(smx_handle h, const smx_agent_entry* entry);
int smx_check_agent_entry(const smx_config* cfg, const smx_agent_entry* entry, char* err, uint64_t err_len);
/* Per-agent action spaces (every agent of the reference brings its own AgentInterface, agent_interface.py:300-330; the
 * controller is chosen per agent, smarts.py:1233-1263 over controllers/__init__.py:61-152).  Opt-in: with nothing bound
 * every agent has cfg.action_space, as before.  space_host[a] is the SMX_ACTION_SPACE_* of agent slot a — the same in
 * every env, as missions and vias are — and the six spaces that drive the Ackermann chassis may be mixed freely: LANE,
 * CONTINUOUS, ACTUATOR_DYNAMIC, LANE_WITH_CONTINUOUS_SPEED, TRAJECTORY, MPC.  They share the state layout, the reset and
 * the observation pass; only the control phase of smx_step_mixed reads the table.  A table whose entries are all equal
 * is legal.  While a table is bound
 *   - smx_step_mixed is the tick; smx_step, smx_step_continuous, smx_step_trajectory, smx_step_target_pose,
 *     smx_step_trajectory_with_time, smx_step_history_agents and smx_step_history_handover return SMX_ERR_STATE (the
 *     message names smx_step_mixed), and so does smx_actions_to_world (ego-frame actions of a mixed fleet are not built);
 *   - smx_set_history_agents, smx_set_history_handover, smx_set_history_bubbles and smx_set_agent_dims return
 *     SMX_ERR_STATE (they need a kinematic cfg.action_space, which a table is refused beside);
 *   - the LARGE launch form is the teams cut, whatever the map (smx_launch_form reports it).
 * Binding and unbinding need no reset: the controller's state words are per agent.  Rebinding in the middle of an episode
 * leaves a slot's controller words (SMX_S_LAT_INT .. SMX_S_SPD_ERR, SMX_S_MCL_X / _Y, SMX_F_MCL_SET) with the meaning
 * its previous space gave them; an smx_reset after rebinding is recommended.
 * Refused (SMX_ERR_INVALID, the reason names the slot): a null table, n_agents != num_vehicles - num_social, an entry that
 * is no SMX_ACTION_SPACE_* or is kinematic (TARGET_POSE, TRAJECTORY_WITH_TIME, IMITATION), a cfg.action_space that is
 * itself kinematic.  The table is copied; spaces = NULL unbinds.  Waits for the device.  smx_check_agent_spaces is the
 * validation alone, without a device or a handle. */
typedef struct smx_agent_spaces {
  const int32_t* space_host;   /* [n_agents] SMX_ACTION_SPACE_* per agent slot; the same in every env */
  int32_t n_agents;            /* must equal num_vehicles - num_social */
} smx_agent_spaces;
int smx_set_agent_spaces(smx_handle h, const smx_agent_spaces* spaces);
int smx_check_agent_spaces(const smx_config* cfg, const smx_agent_spaces* spaces, char* err, uint64_t err_len);
/* Frame stacking (smx_config.frame_stack = k): for every agent the device keeps the last k frames of each bound row,
 * newest first (frame 0 is this pass's row), in a caller-owned device buffer.  At the end of every smx_reset / smx_step*
 * pass, on the caller's stream, once every row of the pass is complete (under auto_reset: after the reset pass has
 * written a restarted env's first observation), each agent's stacks are
 *   pushed  — frames 0..k-2 move to 1..k-1, the row becomes frame 0 (deque.appendleft, frame_stack.py:69-72) — when the
 *             agent had an observation in the tick: alive at the tick's start and not a social slot (the agents whose
 *             rgb / ec_* / lane_ttc rows the pass wrote);
 *   filled  — all k frames become the row (frame_stack.py:104-109) — when the observation is the first of an episode:
 *             the envs smx_reset selects, and under auto_reset an env that restarts inside the launch (the finishing
 *             tick's row is not pushed: ParallelEnv's worker calls the wrapped reset(), parallel_env.py:303-309);
 *   held    — byte for byte — otherwise: an agent that is done while its env goes on, every social slot, the envs a
 *             masked smx_reset leaves alone.  There is no final_* twin.
 * `source`: an SMX_OUT_* index of a per-agent row ([E*N]...), read from the smx_outputs the pass is called with, or
 * SMX_STACK_SOURCE_RGB for the image bound by smx_set_rgb_output when the pass runs (callers may alternate image
 * buffers).  Refused: SMX_OUT_ENV_DONE, SMX_OUT_LEARNER, the SMX_OUT_FINAL_* rows, a row whose sensor is off.
 * `layout`: SMX_STACK_FRAMES = [E*N][k][row...]; SMX_STACK_DSTACK (SMX_STACK_SOURCE_RGB only, 16-byte aligned) =
 * [E*N][H][W][3k], channel 3j + c = frame j's channel c: the array RGBImage.observation returns (rgb_image.py:93-99).
 * `bytes`: what the caller allocated, at least E * N * k * (the row's bytes per agent).  stack_dev = NULL unbinds
 * (source, layout).  At most SMX_STACK_MAX_BINDINGS bindings, one per (source, layout); binding again replaces the
 * buffer.  Errors: SMX_ERR_STATE with frame_stack == 0 or a 17th binding, SMX_ERR_INVALID for a bad source or layout,
 * too few bytes or a misaligned DSTACK buffer; a pass with a bound source whose row pointer is NULL returns
 * SMX_ERR_STATE.  smx_check_frame_stack is the validation alone, callable without a device or a handle (it knows no
 * other bindings): SMX_OK, or the code with the reason in err[err_len]. */
enum { SMX_STACK_SOURCE_RGB = 1 << 16 };
enum { SMX_STACK_FRAMES = 0, SMX_STACK_DSTACK = 1 };
#define SMX_STACK_MAX_FRAMES 8
#define SMX_STACK_MAX_BINDINGS 16
int smx_bind_frame_stack(smx_handle h, int32_t source, int32_t layout, void* stack_dev, uint64_t bytes);
int smx_check_frame_stack(const smx_config* cfg, int32_t source, int32_t layout, uint64_t bytes, char* err, uint64_t err_len);
/* Re-initialise the envs whose mask byte is non-zero (NULL = all) from the spawn
 * table and produce their first observations. */
int smx_reset(smx_handle h, const uint8_t* env_mask_dev, const smx_state* st, const smx_spawns* sp,
              const smx_outputs* out, void* hip_stream);
/* One tick for every env: actions[E*N] are SMX_ACTION_* (int8, device). */
int smx_step(smx_handle h, const int8_t* actions_dev, const smx_state* st, const smx_spawns* sp,
             const smx_outputs* out, void* hip_stream);
/* The same tick for the float action spaces, Imitation among them: actions[E*N][3] (float32, device). */
int smx_step_continuous(smx_handle h, const float* actions_dev, const smx_state* st, const smx_spawns* sp,
                        const smx_outputs* out, void* hip_stream);
/* The following tick of the history agents (smx_set_history_agents, above): no actions. */
int smx_step_history_agents(smx_handle h, const smx_state* st, const smx_spawns* sp, const smx_outputs* out, void* hip_stream);
/* The mixed tick (smx_set_history_handover, above): every agent follows or is driven by actions[E*N][3], as its handover
 * tick says. */
int smx_step_history_handover(smx_handle h, const float* actions_dev, const smx_state* st, const smx_spawns* sp,
                              const smx_outputs* out, void* hip_stream);
/* The same tick for ActionSpaceType.Trajectory and ActionSpaceType.MPC.  trajectories[E*N][4][SMX_TRAJ_COLS] (float64,
 * device): rows x, y, heading, speed; columns 0..9 = the first ten points, column 10 = the LAST point of the
 * trajectory — all the PD controller reads, and all the MPC one does (curvature_calculation at offsets <= 4 over
 * five points reaches index 9, the look-ahead index is min(3 or 1, n - 1), the desired speed is the last point's);
 * counts[E*N] (int32, device) = the trajectory's true length, 0 = no action this tick. */
#define SMX_TRAJ_COLS 11
int smx_step_trajectory(smx_handle h, const double* trajectories_dev, const int32_t* counts_dev, const smx_state* st,
                        const smx_spawns* sp, const smx_outputs* out, void* hip_stream);
/* The same tick for ActionSpaceType.TargetPose.  targets[E*N][4] (float64, device): x, y, heading, seconds into the
 * future at which the pose is wanted; a NaN x = no action this tick (the provider then aims at the pose it holds). */
int smx_step_target_pose(smx_handle h, const double* targets_dev, const smx_state* st, const smx_spawns* sp,
                         const smx_outputs* out, void* hip_stream);
/* The same tick for ActionSpaceType.TrajectoryWithTime.  trajectories[E*N][5][max_points] (float64, device): rows time,
 * x, y, heading, speed; counts[E*N] (int32, device) = points given, 0 = no action this tick (the vehicle is not
 * updated at all). */
int smx_step_trajectory_with_time(smx_handle h, const double* trajectories_dev, const int32_t* counts_dev,
                                  int32_t max_points, const smx_state* st, const smx_spawns* sp, const smx_outputs* out,
                                  void* hip_stream);
/* The tick of a mixed fleet (smx_set_agent_spaces, above): every agent slot is stepped by the controller of its own
 * space, from the buffer of that space's kind, each laid out over all E*N vehicles as its uniform entry has it.  "No
 * action" keeps each space's convention: code -1, a NaN first float, count 0.  A Lane code outside -1..3 is reported by
 * smx_sync for Lane slots only (no other slot's byte is read).  The buffer of a space the table does not hold may be
 * NULL and is never read; SMX_ERR_INVALID when the buffer of a space it holds is NULL, SMX_ERR_STATE when no table is
 * bound.  One launch (small form) or pair of launches (large form, lane spaces) per space present, all on hip_stream;
 * the social slots are stepped once, by the launch of the lowest-numbered space present. */
typedef struct smx_mixed_actions {
  const int8_t*  lane_dev;          /* [E*N], as smx_step: read for Lane slots                                   */
  const float*   floats_dev;        /* [E*N][3], as smx_step_continuous: Continuous / ActuatorDynamic / LWCS slots */
  const double*  trajectories_dev;  /* [E*N][4][SMX_TRAJ_COLS] and                                               */
  const int32_t* counts_dev;        /* [E*N], as smx_step_trajectory: Trajectory / MPC slots                     */
} smx_mixed_actions;
int smx_step_mixed(smx_handle h, const smx_mixed_actions* acts, const smx_state* st, const smx_spawns* sp,
                   const smx_outputs* out, void* hip_stream);
/* The action half of the ego-centric adapters (ego_centric_adapters.py:195-266): rewrites an action buffer given in the
 * frame of each agent's last observation (out->ego_frame, out->ec_flags: the last smx_reset / smx_step* pass) into
 * out_dev, a second caller-owned device buffer of the same layout, which the matching smx_step_* then takes.  One
 * kernel on hip_stream, no synchronisation.  With (px, py, pz, H) the frame, to_world(q) = inv(M) q + (px, py, pz)
 * (world_position_from_ego_frame, math.py:490-505; inv(M) is M's transpose) and headings become
 * wrap_value(h + H, -pi, pi) (no Heading()):
 *   SMX_ACTION_SPACE_TRAJECTORY, _MPC      [E*N][4][SMX_TRAJ_COLS]: columns < min(count, 10) and column 10; speed copied
 *   SMX_ACTION_SPACE_TARGET_POSE           [E*N][4]: x, y, heading; seconds copied (counts_dev is not read)
 *   SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME  [E*N][5][max_points]: rows 1, 2, 3 (x, y, heading) of the first
 *                                          min(count, max_points) points; time and speed copied
 * (the rows smx_step_trajectory_with_time calls x, y and heading; the reference's adapter would rotate rows 0 and 1,
 * DESIGN.md).  Every other element is copied.  An agent is copied through whole when its ec_flags is 0 (last_obs is
 * None), when it sent no action (NaN x, count 0) or when it is a social slot.  action_space must be one of the four
 * and equal cfg.action_space (else SMX_ERR_INVALID; Imitation actions hold no position or heading and pass through
 * the reference's adapter unchanged); a configuration without SMX_SENSOR_EGO_CENTRIC gives SMX_ERR_STATE. */
int smx_actions_to_world(smx_handle h, int32_t action_space, const double* in_dev, const int32_t* counts_dev,
                         int32_t max_points, double* out_dev, const smx_outputs* out, void* hip_stream);
/* Waits for the stream, then reports what only the kernels could see since the last smx_sync, as SMX_ERR_INVALID: a
 * Lane action code outside -1..3; a TrajectoryWithTime action the reference raises on (fewer than two points or more
 * than max_points, a value that is not finite, times not strictly increasing, no point later than dt or the first one
 * already later); a TargetPose action that yields a pose that is not finite; an Imitation action with a finite first
 * float and an infinite second one, or one that yields a pose or a speed that is not finite.  Such an agent is stepped
 * as if it had sent no action. */
int smx_sync(smx_handle h, void* hip_stream);
/* Device-side timing: while enabled, every smx_step is bracketed by a hipEvent pair recorded on
 * the stream it is launched on (no synchronisation).  smx_read_step_ms waits for the recorded
 * launches, writes their durations (milliseconds, oldest first, at most `max`) and clears the
 * log; *n receives the count.  smx_last_step_ms is the single-launch convenience form.
 *
 * Levels: 0 = off; 1 = one event pair around the whole smx_step (the bench's timed region uses
 * this); 2 = a boundary event after every kernel of the tick, read back per phase with
 * smx_read_phase_ms as ms[n][SMX_PHASE_COUNT] (a phase whose sensor is disabled reads ~0). */
enum {
  SMX_PHASE_CONTROL = 0, /* k_control: controllers + vehicle dynamics (a1-a6)            */
  SMX_PHASE_SCAN,        /* k_scan: road facts + lanepoint seeds (a8, a9 front half)      */
  SMX_PHASE_OGM,         /* k_ogm (a14), k_dagm and k_rgb                                 */
  SMX_PHASE_SENSORS,     /* k_sensors: waypoints | observe | lidar roles (a7, a9-a13, a15) */
  SMX_PHASE_COMMIT,      /* k_commit: flags, env done count, auto-reset respawn           */
  SMX_PHASE_RESET,       /* auto-reset pass (parallel_env.py:303-309), all kernels        */
  SMX_PHASE_COUNT
};
int smx_set_timing(smx_handle h, int level);
int smx_read_phase_ms(smx_handle h, float* ms, int32_t max_steps, int32_t* n);
int smx_read_step_ms(smx_handle h, float* ms, int32_t max, int32_t* n);
int smx_last_step_ms(smx_handle h, float* ms);
const char* smx_last_error(smx_handle h);
/* sizeof() of the ABI structs as compiled (0 config, 1 map tables, 2 state, 3 spawns, 4 outputs):
 * lets a foreign-language binding verify its mirror of the layouts. */
uint64_t smx_struct_size(int which);
/* Lateral gains of the lane-following controller for target_speed > 0
 * (lane_following_controller.py:420-430); defaults are the sedan's clip bounds (0.04, 3.4). */
int smx_set_controller_gains(smx_handle h, double heading_gain, double lateral_gain);
/* How a tick is cut into launches.  The same role functions run either way and the results are the same;
 * the forms differ in what bounds them.  SMALL: few launches whose workgroups take different roles (a batch
 * that cannot fill the chip is bound by one wavefront's latency); LARGE: one launch per role, waypoint rows
 * emitted in memory order from LDS knot tables (bound by throughput).  AUTO picks by vehicle count. */
enum { SMX_LAUNCH_AUTO = 0, SMX_LAUNCH_SMALL = 1, SMX_LAUNCH_LARGE = 2,
       SMX_LAUNCH_LARGE_ONE_LANE = 3, SMX_LAUNCH_LARGE_TEAMS = 4 /* a cut of LARGE forced, whatever the map and the size (smx_launch_form) */ };
int smx_set_launch_strategy(smx_handle h, int strategy);
/* The form the next tick will run in (after smx_load_map): the LARGE form comes in two cuts — one lane per vehicle
 * seeded by last tick's answers with the rare cases on device-side slow lists, where the map's lanes never split
 * (no lanepoint with several successors: loop), and teams of lanes per vehicle for everybody where they do
 * (intersections, minicity: a third of the vehicles would be "rare cases").  Inside the one-lane cut the path-seeds
 * search is the one-lane kernel from 114 688 vehicles on and the team kernel below (its slow chain's latency would
 * end the tick of a smaller batch).  Same results either way. */
enum { SMX_FORM_SMALL = 0, SMX_FORM_LARGE_TEAMS = 1, SMX_FORM_LARGE_ONE_LANE = 2 };
int smx_launch_form(smx_handle h);
/* The OGM rows (smx_outputs.ogm) and the pieces the handle knows to be zero in them.  smx_invalidate_outputs: the caller
 * wrote into the rows itself, the next call stores whole tiles.  smx_set_ogm_delta: on (the default) stores only the
 * pieces that changed; off stores every piece in every call, and the rows may then be written freely. */
int smx_invalidate_outputs(smx_handle h);
int smx_set_ogm_delta(smx_handle h, int on);
const char* smx_version(void);
void smx_destroy(smx_handle h);

#ifdef __cplusplus
}
#endif
#endif /* SMX_H */
