/* rbp_host.h — host-side front-end (the callers / data formats either side of the hot path).
 *
 * Not accelerated; exists so that mission JSONs and octomap .bt worlds can be fed to rbp.h without ROS,
 * octomap, dynamicEDT3D or Boost:
 *   Mission::setMission            swarm_planner/include/mission.hpp:22-88
 *   octomap::OcTree(path) + DynamicEDTOctomap(1, tree, min, max, false).update()
 *                                  swarm_planner/src/swarm_traj_planner_rbp_test_all.cpp:51-63
 *   ECBSPlanner::update            swarm_planner/include/ecbs_planner.hpp:21-136
 * Plain C ABI; buffers returned by the _load/_build calls are owned by the library and freed by the matching _free.
 */
#ifndef RBP_HOST_H
#define RBP_HOST_H

#include "rbp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mission JSON ({"quadrotors": {...}, "agents": [...]}), mission.hpp:22-88 ---------------- */
typedef struct rbp_mission_buf {
    int32_t N;
    double* start;   /* [N][9] */
    double* goal;    /* [N][9] */
    double* radius;  /* [N] */
    double* speed;   /* [N]  quad_speed (parsed, unused by the path) */
    double* max_vel; /* [N][3] */
    double* max_acc; /* [N][3] */
} rbp_mission_buf;
int rbp_mission_load_json(const char* path, rbp_mission_buf* out);
void rbp_mission_free(rbp_mission_buf* m);

/* ---- octomap .bt reader: occupied leaves (a leaf above depth 16 is a cube of `size` voxels per edge) */
typedef struct rbp_octomap_buf {
    double res;
    int64_t n_occupied;   /* occupied leaves */
    int32_t* keys;        /* [n_occupied][4] = min-corner voxel key minus 32768 (x,y,z), edge length in voxels */
    int64_t n_nodes;      /* node count as parsed (equals the header's `size`) */
} rbp_octomap_buf;
int rbp_octomap_load_bt(const char* path, rbp_octomap_buf* out);
void rbp_octomap_free(rbp_octomap_buf* m);

/* ---- distance map over the world bounding box (exact EDT in cells, clamped like dynamicEDT3D) -- */
typedef struct rbp_world_buf {
    int32_t dim[3];
    int32_t key_min[3];
    double res;
    float* dist;          /* [nx][ny][nz] metres */
} rbp_world_buf;
/* bbx_min/bbx_max are converted to float first (octomap::point3d), as the reference does. max_dist in metres. */
int rbp_world_build(const rbp_octomap_buf* map, const double bbx_min[3], const double bbx_max[3], double max_dist,
                    rbp_world_buf* out);
void rbp_world_free(rbp_world_buf* w);

/* ---- ECBS front-end: initTraj [N][M+1][3] float32 and T[M+1] (ecbs_planner.hpp:34-70) --------- */
typedef struct rbp_init_traj_buf {
    int32_t N, M;
    double* T;            /* [M+1] */
    float* init_traj;     /* [N][M+1][3] */
    int32_t makespan;     /* max path cost */
    int32_t sum_cost;
    int64_t high_level_expanded;
    int64_t low_level_expanded;
} rbp_init_traj_buf;
/* returns 0 ok; 1 start/goal occluded; 2 search failed / node budget exhausted */
int rbp_ecbs_plan(const rbp_world_buf* world, const rbp_mission* mission, const rbp_param* param,
                  int64_t max_high_level_nodes, rbp_init_traj_buf* out);
/* rbp_ecbs_plan in its two halves -- the same result as the one call, which is the two composed:
 * rbp_ecbs_obstacles: ECBSPlanner::setObstacles (ecbs_planner.hpp:80-109), the only reader of the fine grid: the planning lattice's shape in
 *   dim and, if obstacle != NULL (capacity >= dim[0]*dim[1]*dim[2] bytes), its occupancy mask [dimx][dimy][dimz] of 0 / 1.  Returns 0 ok;
 *   1 a sample of the lattice lies outside the world's grid (the mask is then incomplete); RBP_ERR_BAD_ARGUMENT.  A world that lives on
 *   the GPU gives the same mask through rbp_dev_worlds_ecbs_obstacles of rbp.h.
 * rbp_ecbs_plan_obstacles: the search on such a mask (dim must be the lattice's shape for `param`); returns as rbp_ecbs_plan. */
int rbp_ecbs_obstacles(const rbp_world_buf* world, const rbp_mission* mission, const rbp_param* param, int32_t dim[3], uint8_t* obstacle,
                       size_t capacity);
int rbp_ecbs_plan_obstacles(const int32_t dim[3], const uint8_t* obstacle, const rbp_mission* mission, const rbp_param* param,
                            int64_t max_high_level_nodes, rbp_init_traj_buf* out);
void rbp_init_traj_free(rbp_init_traj_buf* t);

/* ---- validation metrics of rbp_publisher.hpp:685-695, 769-798 ------------------
 * coef as in rbp_plan.coef.  dt = sampling step (reference: 0.1 s). */
int rbp_validate(const rbp_mission* mission, const rbp_param* param, int32_t M, const double* T, const double* coef,
                 double dt, double* min_safety_ratio, double* total_flight_distance);

/* The same two signals as an rbp_report (rbp.h), by the rule of csrc/common/report_rules.h that the device shares: what
 * rbp_session_report / rbp_dev_report return for the same plan, bit for bit, and their reference.  Same inputs as rbp_validate (T as
 * downloaded, i.e. scaled); it differs from rbp_validate by rounding only -- Horner instead of std::pow, the distance summed per agent and
 * then over the agents -- and also says at which (sample, qi, qj) the minimum lies.  out->status is 0. */
int rbp_report_host(const rbp_mission* mission, const rbp_param* param, int32_t M, const double* T, const double* coef,
                    double dt, rbp_report* out);

/* The sampled states, limit peaks and ratio curves of one plan as an rbp_dynamics (rbp.h), by the sequential loop of
 * csrc/common/state_rules.h that the device shares: what rbp_session_dynamics / rbp_dev_dynamics return for the same plan, bit for bit,
 * and their reference.  T as downloaded (scaled); max_vel / max_acc are the mission's.  states [N][9][S_stride] and curves [S_stride][2]
 * may each be NULL; they are written only where samples <= S_stride (out->stored), entries beyond `samples` stay.  out->status is 0. */
int rbp_dynamics_host(const rbp_mission* mission, const rbp_param* param, int32_t M, const double* T, const double* coef,
                      double dt, rbp_dynamics* out, double* states, double* curves, int32_t S_stride);

/* The clearance of one plan to the obstacles of its world as an rbp_clearance (rbp.h), by the sequential loop of
 * csrc/common/clearance_rules.h that the device shares: what rbp_session_clearance / rbp_dev_clearance return for the same plan and grid,
 * bit for bit, and their reference.  world->dist is a host grid; T as downloaded (scaled); radius is the mission's.  agent_clearance [N]
 * may be NULL; it is written only where the samples are evaluated (out->samples >= 0).  out->status is 0. */
int rbp_clearance_host(const rbp_world* world, const rbp_mission* mission, int32_t M, const double* T,
                       const double* coef, double dt, rbp_clearance* out, double* agent_clearance /* [N] or NULL */);

/* The certified interval of one plan's smallest safety ratio in continuous time as an rbp_separation (rbp.h), by the sequential loop of
 * csrc/common/separation_rules.h that the device shares: what rbp_session_separation / rbp_dev_separation return for the same plan, bit
 * for bit, and their reference.  T as downloaded (scaled); radius is the mission's, the downwash param's.  depth in
 * 0 .. RBP_SEPARATION_MAX_DEPTH and refine_below > 0, otherwise RBP_ERR_BAD_ARGUMENT.  pair_lower [N (N-1) / 2] may be NULL.
 * out->status is 0. */
int rbp_separation_host(const rbp_mission* mission, const rbp_param* param, int32_t M, const double* T, const double* coef,
                        int32_t depth, double refine_below, rbp_separation* out, double* pair_lower /* [N (N-1) / 2] or NULL */);

/* The certified interval of one plan's smallest clearance to the obstacles of `world` in continuous time as an rbp_swept_clearance (rbp.h),
 * by the sequential loop of csrc/common/swept_rules.h that the device shares: what rbp_session_swept_clearance / rbp_dev_swept_clearance
 * return for the same plan and grid, bit for bit, and their reference.  T as downloaded (scaled); radius is the mission's; world->dist a
 * host grid.  depth in 0 .. RBP_SWEPT_MAX_DEPTH and refine_below a number, otherwise RBP_ERR_BAD_ARGUMENT.  agent_lower [N] may be NULL.
 * out->status is 0. */
int rbp_swept_clearance_host(const rbp_world* world, const rbp_mission* mission, int32_t M, const double* T, const double* coef,
                             int32_t depth, double refine_below, rbp_swept_clearance* out, double* agent_lower /* [N] or NULL */);

/* The certified intervals of one plan's largest velocity and acceleration, as fractions of the mission's max_vel / max_acc, in continuous
 * time as an rbp_limits (rbp.h), by the sequential loop of csrc/common/limits_rules.h that the device shares: what rbp_session_limits /
 * rbp_dev_limits return for the same plan, bit for bit, and their reference.  T as downloaded (scaled).  depth in
 * 0 .. RBP_LIMITS_MAX_DEPTH and refine_above a number, otherwise RBP_ERR_BAD_ARGUMENT.  agent_upper [N][2] may be NULL.  out->status is 0. */
int rbp_limits_host(const rbp_mission* mission, int32_t M, const double* T, const double* coef, int32_t depth, double refine_above,
                    rbp_limits* out, double* agent_upper /* [N][2] or NULL */);

/* crazyswarm CSV of rbp_planner.hpp:295-324 (one file per agent: <dir>/coef<qi+1>.csv) */
int rbp_write_coef_csv(const char* dir, int32_t N, int32_t M, const double* T, const double* coef);

/* The QP of batch `l` as a CPLEX LP-format file: what cplex.exportModel(".../log/QPmodel.lp") writes when the reference runs with
 * log = true (rbp_planner.hpp:150-152): variables named and ordered as in populatebyrow (:552-577), objective without 1/2,
 * equality, SFC and RSFC rows (:582-684).  plan: T / init_traj / corridor as BEFORE timeScale.  dummy: the control points frozen
 * agents are held at ([N][3][6M], the layout of rbp_plan.ctrl), or NULL for build_dummy of the initial trajectory (:513-549). */
int rbp_write_qp_lp(const char* path, const rbp_mission* mission, const rbp_param* param, const rbp_plan* plan, int32_t l,
                    const double* dummy);

#ifdef __cplusplus
}
#endif
#endif
