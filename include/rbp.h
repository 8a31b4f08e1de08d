/* rbp.h — C ABI of the MI355X-native RBP plan path (SFC + RSFC + QP).
 *
 * This is the drop-in boundary for the two header-only C++ stages of the reference
 *   SwarmPlanning::Corridor::update(bool, PlanResult*)    swarm_planner/include/rbp_corridor.hpp:21-26
 *   SwarmPlanning::RBPPlanner::update(bool, PlanResult*)  swarm_planner/include/rbp_planner.hpp:33-84
 * The reference has no FFI; the shared state between the stages is `PlanResult`
 * (swarm_planner/include/sp_const.hpp:21-28).  Here the same state is a set of caller-owned flat
 * arrays (`rbp_plan`), the distance map is a flat float grid (`rbp_world`, what
 * DynamicEDTOctomap::getDistance serves in rbp_corridor.hpp:66) and Mission/Param are plain structs
 * (mission.hpp:13-15, param.hpp:44-70).  INTEGRATION.md shows the ~80-line adapter a maintainer of
 * the reference would add.
 *
 * All pointers are HOST pointers unless a function says otherwise.  Plain C, no torch types.
 */
#ifndef RBP_H
#define RBP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (the reference returns bool + ROS_ERROR; 0 == true) ------------------------- */
enum {
    RBP_OK = 0,
    RBP_ERR_OBSTACLE_IN_INIT_TRAJ = 1, /* rbp_corridor.hpp:181-187 "Obstacle invades initial trajectory" */
    RBP_ERR_UNEQUAL_TRAJ_LEN = 2,      /* rbp_corridor.hpp:346-349 (cannot happen with the flat layout; kept) */
    RBP_ERR_INIT_TRAJ_COLLIDE = 3,     /* rbp_corridor.hpp:385-388 "initial trajectories are collided" */
    RBP_ERR_SFC_OVERFLOW = 4,          /* more boxes than plan->max_boxes (flat-layout only) */
    RBP_ERR_QP_FAILED = 10,            /* rbp_planner.hpp:158-161 "Failed to optimize QP" (infeasible / no convergence) */
    RBP_ERR_UNSUPPORTED_DEGREE = 11,   /* rbp_planner.hpp:344-346, 375-377: only n=5, phi=3 */
    RBP_ERR_BAD_ARGUMENT = 20,
    RBP_ERR_NO_DEVICE = 30,            /* HIP device / kernel image unavailable: the product path never falls back to CPU */
    RBP_ERR_HIP = 31,
    RBP_ERR_EXCHANGE = 32              /* rbp_session_shard_joint: the caller's exchange hook reported a failure */
};

/* ---- distance map: what DynamicEDTOctomap(maxDist=1, tree, bbxMin, bbxMax, false) serves -------
 * swarm_planner/src/swarm_traj_planner_rbp.cpp:73-80.  Cell (ix,iy,iz) holds the voxel whose octomap key
 * (minus 32768) is key_min + (ix,iy,iz); a point p maps to key floor((1/res) * (double)p) per axis and
 * reads -1 outside the grid (so out-of-world samples count as obstacle in rbp_corridor.hpp:67). */
typedef struct rbp_world {
    int32_t dim[3];     /* nx, ny, nz */
    int32_t key_min[3]; /* voxel key of cell (0,0,0), relative to the octree centre */
    double res;         /* octree resolution [m] */
    const float* dist;  /* [nx][ny][nz], metres, z fastest; a host pointer, or a DEVICE pointer (see below) */
} rbp_world;
/* rbp_world.dist may point into the HBM of the device the call runs on -- a grid of rbp_dev_worlds (below), or any other device
 * allocation of that layout, e.g. a caller's torch tensor -- wherever a world is taken: rbp_session_create / rbp_session_create_in,
 * the one-shot and context calls, rbp_corridor_update_range.  The library asks the HIP runtime what the pointer is (a pointer the
 * runtime does not know is a host pointer).  A device grid is referenced IN PLACE: nothing is copied, so the caller keeps it alive
 * and unchanged until the session is destroyed (the one-shot and context calls: until they return).  A grid on another device than
 * the session's is RBP_ERR_BAD_ARGUMENT.  Missions that hand in the same pointer and shape share one grid, host or device. */

/* ---- mission.hpp:13-15 ---------------------------------------------------------------------- */
typedef struct rbp_mission {
    int32_t N;             /* qn */
    const double* start;   /* [N][9]  pos(3) vel(3) acc(3)   mission.hpp:47-53 */
    const double* goal;    /* [N][9]                         mission.hpp:55-61 */
    const double* radius;  /* [N]     quad_size              mission.hpp:64 */
    const double* max_vel; /* [N][3]                         mission.hpp:70-76 */
    const double* max_acc; /* [N][3]                         mission.hpp:78-83 */
} rbp_mission;

/* ---- param.hpp:44-70 (names and defaults are the reference's) -------------------------------- */
typedef struct rbp_param {
    double world_min[3]; /* world/x_min,y_min,z_min  (-5,-5,0)   */
    double world_max[3]; /* world/x_max,y_max,z_max  (5,5,2.5)   */
    double box_xy_res;   /* box/xy_res 0.1 */
    double box_z_res;    /* box/z_res  0.1 */
    double downwash;     /* plan/downwash 2.0 */
    double time_step;    /* plan/time_step 1 */
    double ecbs_w;       /* ecbs/w 1.3        (front-end only) */
    double grid_xy_res;  /* grid/xy_res 0.3   (front-end only) */
    double grid_z_res;   /* grid/z_res 0.6    (front-end only) */
    double grid_margin;  /* grid/margin 0.2   (front-end only) */
    int32_t n;           /* plan/n 5   */
    int32_t phi;         /* plan/phi 3 */
    int32_t sequential;  /* plan/sequential false */
    int32_t batch_size;  /* plan/batch_size 4 */
    int32_t batch_iter;  /* plan/batch_iter 0 (launch files pass -1 = all batches) */
    int32_t iteration;   /* plan/iteration 1 */
    int32_t time_scale;  /* plan/time_scale true */
    int32_t log;         /* log false */
    int32_t timescale_rule; /* NOT a key of the reference (ABI 6): which candidate times timeScale's velocity check inspects -- see below */
} rbp_param;

/* rbp_param.timescale_rule.  scale_to_max_vel (rbp_planner.hpp:756-794) evaluates |velocity| at t = 0, t = dt and at the roots
 * roots_derivative(2, coef_der) returns (:727-754): eigenvalues of the cubic's companion matrix from Eigen::EigenSolver, of which the loop
 * `for (j = 0; j < i; j++)` (:746, i = 2 = the derivative order) reads only the FIRST TWO, in Eigen's internal order.
 *   RBP_TIMESCALE_ALL_REAL_ROOTS (0, the default): every real root of the cubic is a candidate.  The factor can only be >= the reference's
 *     (more candidates), is still a power of 1.1, and respects max_vel at EVERY velocity extremum -- the reference's literal rule can leave
 *     a segment above max_vel when the skipped third eigenvalue holds the peak.  Independent of any eigenvalue ordering.
 *   RBP_TIMESCALE_FIRST_EIGENVALUES (1): the loop as written -- the real ones among the first two eigenvalues, in the order of the real
 *     Schur decomposition of Eigen 3.3.x (Francis double-shift QR on the companion matrix, eigenvalues read off T from the top), restated
 *     from Eigen's published algorithm in kernels/qp.hip; Eigen is an un-pinned system dependency of the reference, so this order is a
 *     documented, deterministic choice, not a pinned one.
 * Both factors are always computed: rbp_plan.time_scale is the selected rule's (and what coef / T / corridor times are scaled by),
 * rbp_plan.time_scale_alt the other rule's -- `time_scale != time_scale_alt` tells a caller that the two rules disagree on this plan
 * (6 of 150 cases on the 50-map sweep with limits scaled by 1 / 0.5 / 0.25, each time by one step of the 1.1 ladder:
 * tests/test_timescale_rule.py). */
enum { RBP_TIMESCALE_ALL_REAL_ROOTS = 0, RBP_TIMESCALE_FIRST_EIGENVALUES = 1 };

/* Fill `p` with the defaults of Param::setROSParam (param.hpp:44-70). */
void rbp_param_defaults(rbp_param* p);

/* ---- PlanResult (sp_const.hpp:21-28) as flat caller-owned arrays ------------------------------
 * pair index of (qi<qj):  qi*N - qi*(qi+1)/2 + (qj-qi-1)   (the order RSFC[qi][qj] is filled in
 * rbp_corridor.hpp:342-344). */
typedef struct rbp_plan {
    int32_t N;              /* agents (== mission.N) */
    int32_t M;              /* segments = T.size()-1            rbp_planner.hpp:35 */
    double* T;              /* [M+1] segment times; rescaled in place by time_scale (rbp_planner.hpp:262-264) */
    const float* init_traj; /* [N][M+1][3] float32 = octomap::point3d waypoints (sp_const.hpp:16) */

    /* SFC_t (sp_const.hpp:17): per agent a list of (box[6] = xmin,ymin,zmin,xmax,ymax,zmax ; end time) */
    int32_t max_boxes;      /* capacity per agent; M always suffices */
    int32_t* sfc_count;     /* [N] */
    double* sfc_box;        /* [N][max_boxes][6] */
    double* sfc_time;       /* [N][max_boxes]     rescaled by time_scale (rbp_planner.hpp:250-252) */

    /* RSFC_t (sp_const.hpp:18): per pair and segment (float32 normal ; time T[m+1]) */
    float* rsfc_normal;     /* [N(N-1)/2][M][3] */
    double* rsfc_time;      /* [M]  (= T[1..M], identical for every pair; rescaled like rbp_planner.hpp:255-258) */

    /* RBPPlanner outputs */
    double* coef;           /* [N][3][6M]: per agent the column-major (6M x 3) matrix the reference copies into
                               msgs_traj_coef[qi].data (rbp_planner.hpp:286-289); rows m*6+i hold the coefficient of
                               (t-T_m)^(5-i), i.e. descending powers, seconds (rbp_planner.hpp:170-186) */
    double* ctrl;           /* [N][3][6M] Bernstein control points (the reference's `dummy`/`vals`), may be NULL */
    double time_scale;      /* rbp_planner.hpp:235 */
    double total_cost;      /* "QP total cost" rbp_planner.hpp:205: sum of batch objectives of the last pass */
    int32_t x_size;         /* count_x  of the last batch  rbp_planner.hpp:58 */
    int32_t eq_size;        /* count_eq                    rbp_planner.hpp:59 */
    int32_t ineq_size;      /* count_lq                    rbp_planner.hpp:60 */
    int32_t qp_iterations;  /* total interior-point iterations spent (diagnostic, not in the reference) */
    /* solver outcome (not in the reference, where cplex.solve() either returns an optimum or throws, rbp_planner.hpp:158-161):
     * every batch QP ends with an active-set polish whose answer is accepted only under a full KKT check; a QP whose polish
     * was refused keeps the interior-point answer (optimal to ~1e-5 m instead of ~1e-8 m) and is counted here */
    int32_t qp_solves;      /* batch QPs solved (passes x batches) */
    int32_t qp_unpolished;  /* of those, how many kept the interior-point answer; 0 = every answer is a certified optimum */
    double kkt_max;         /* max over the batch QPs of the accepted answer's KKT residual: polished QPs max(row violation [m],
                               -min multiplier / max(1, max multiplier)); unpolished QPs max(primal residual [m], relative dual
                               residual, complementarity mu) */
    double time_scale_alt;  /* (ABI 6) the factor the OTHER rule of rbp_param.timescale_rule gives for this plan; != time_scale: the rules disagree */
} rbp_plan;

/* ---- the two stage calls (synchronous; results on return) -------------------------------------
 * Corridor::update: reads world, mission.radius, param.{world_*,box_*,downwash}, plan.{T,init_traj};
 * writes plan.{sfc_*, rsfc_*}.  Unlike the reference (which appends, rbp_corridor.hpp:153,190) the
 * outputs are overwritten. */
int rbp_corridor_update(const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan);

/* Agent-sharded Corridor::update for ONE large mission spread over several GPUs (one process per GPU): computes the SFC
 * of agents qi in [agent_begin, agent_end) (the loop body of updateObsBox, rbp_corridor.hpp:154-239) and the RSFC rows
 * of the pairs (qi, qj), qi < qj, with qi in that range (updateRelBox, :342-392); rsfc_time is written by every shard.
 * All other entries of plan.{sfc_*, rsfc_normal} are unspecified: the caller exchanges the shards (all-gather over
 * RCCL/xGMI, swarm_simulator_amd/sharded.py) and obtains exactly what rbp_corridor_update would have written.  Runs on
 * the calling thread's current HIP device. */
int rbp_corridor_update_range(const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan,
                              int32_t agent_begin, int32_t agent_end);

/* RBPPlanner::update: reads mission, param, plan.{T,init_traj,sfc_*,rsfc_*}; writes plan.{coef,ctrl,
 * time_scale,total_cost,*_size} and rescales T / sfc_time / rsfc_time when time_scale != 1. */
int rbp_planner_update(const rbp_mission* mission, const rbp_param* param, rbp_plan* plan);

/* ---- device-resident, batched form (what bench.py times) --------------------------------------
 * A session owns the HBM copies of K independent missions (e.g. the 50-map sweep of
 * swarm_traj_planner_rbp_test_all.cpp:49-103).  `run` only enqueues kernels on `stream`
 * (a hipStream_t passed as void*; NULL = default stream) and never synchronises -- with ONE exception: the PLANNER stage of a
 * non-sequential plan (plan/sequential = false, the reference's code default param.hpp:67: one joint QP over all agents,
 * rbp_planner.hpp:857-859) with rbp_solver_opts.joint_wide_min_agents (16) agents or more runs on the grid-wide solver
 * (kernels/jqp.hip: a launch per phase of the interior-point method over all CUs), whose host loop learns once per iteration whether
 * any mission is still running: that `run` SYNCHRONISES `stream` before it returns. */
typedef struct rbp_session rbp_session;

enum { RBP_STAGE_CORRIDOR = 1, RBP_STAGE_PLANNER = 2, RBP_STAGE_ALL = 3 };

/* ---- solver options (ABI 4) --------------------------------------------------------------------
 * What a caller may legitimately choose about HOW the QPs are solved (never WHAT is computed: every setting ends in the same
 * KKT-verified optimum or the same error).  The library reads NO environment variables: these options are the only switches.
 * Fill the struct with rbp_solver_opts_defaults, change fields, hand it to a session (before its first `run`) or to a context
 * (sessions and one-shot calls made in it inherit the options; ctx == NULL: the calling thread's default context). */
typedef struct rbp_solver_opts {
    int32_t size;                  /* sizeof(rbp_solver_opts) of the caller's header (set by rbp_solver_opts_defaults; checked) */
    int32_t polish;                /* 1: every QP ends with the active-set polish (the certified optimum); 0: the interior-point answer
                                      with its reported KKT residual (diagnostics) */
    int32_t joint_wide_min_agents; /* 16: a joint QP (plan/sequential = false) of at least this many agents runs on the grid-wide
                                      solver (kernels/jqp.hip, no limit on N, `run` synchronises -- rbp_session_run_async does not); fewer agents -- or 0 = never --
                                      run on one workgroup per mission (<= 64 agents, `run` only enqueues) */
    int32_t joint_corrector;       /* 1: one centrality corrector per interior-point iteration of the grid-wide solver */
    int32_t joint_schedule;        /* 0: automatic; 1: look-ahead tile sweep (few missions); 2: bulk tile sweep (many missions); 3: bulk with
                                      two pivot tiles per pass over a knot's matrix (half the HBM traffic of the update; pays only with
                                      hundreds of resident missions: DESIGN.md 3.5) */
    int32_t qp_schedule;           /* batch QPs of the sequential schedule: 0 automatic; 1: one workgroup per mission runs everything
                                      (qp_batch_kernel).  2 was the phase split (chip-wide row sweeps as kernels of their own):
                                      retired, it lost every comparison (docs/HISTORY.md r05); accepted here, refused by a PLANNER run */
    int32_t qp_variant;            /* qp_schedule 1: 0 automatic; 2: 512 threads, one workgroup per CU; 4: 256 threads, two per CU */
    int32_t qp_block_order;        /* qp_schedule 1: 1 = a session that is run again starts its longest missions first; 0 = plain order */
    int32_t qp_groups;             /* reserved (a knob of the retired qp_schedule 2): >= 0, otherwise ignored */
    int32_t qp_rounds;             /* reserved (a knob of the retired qp_schedule 2): >= 0, otherwise ignored */
    double qp_far_slack;           /* qp_schedule 1, first Gauss-Seidel pass, polish on: 0.7 [m].  The interior-point phase of a batch QP leaves
                                      out the frozen-neighbour rows whose slack at the starting point exceeds this for a whole (agent, segment)
                                      group; the polish verifies EVERY row, and a batch QP that does not end polished on the reduced set is
                                      solved again with every row -- the answer is the same certified optimum for any value.  <= 0: off */
} rbp_solver_opts;
void rbp_solver_opts_defaults(rbp_solver_opts* o);

/* worlds/missions/plans: arrays of K structs (host side).  All plans share N; every mission keeps its own M (= ECBS makespan
 * + 2, ecbs_planner.hpp:41-43) and max_boxes, exactly as the reference's map sweep plans each map with its own M. */
int rbp_session_create(rbp_session** out, int device, int K, const rbp_world* worlds, const rbp_mission* missions,
                       const rbp_param* param, const rbp_plan* plans);
int rbp_session_run(rbp_session* s, int stages, void* stream);
/* `run` only enqueues on `stream`, with ONE exception: the PLANNER stage of a joint plan on the grid-wide solver (kernels/jqp.hip,
 * rbp_solver_opts.joint_wide_min_agents), whose host loop learns once per interior-point round whether any mission still iterates --
 * there `run` returns when the solve has ended.  rbp_session_run_async is the same call without that exception: the stages before the
 * joint solve are enqueued on `stream`, the solve itself proceeds on a thread and a stream of the session's own (ordered after `stream`'s
 * work so far by an event), and the call returns at once -- the caller overlaps it with host work (the next mission's ECBS) or with
 * other sessions.  Every later call on the session (download, counters, scalars, reset, run, destroy ...) first waits for the solve;
 * rbp_session_wait does only that and returns the solve's status.  What the caller enqueues on `stream` itself after run_async is NOT
 * ordered after the solve.  For every other session rbp_session_run_async is rbp_session_run. */
int rbp_session_run_async(rbp_session* s, int stages, void* stream);
int rbp_session_wait(rbp_session* s);
/* ---- ONE joint QP on TWO GPUs (ABI 5; BASELINE.json config 4 "agents sharded across GPUs") -------------------------
 * The pair rows of the joint QP couple every agent with every other (rbp_planner.hpp:638-684), so the QP does not split by agent; what
 * splits is its Newton system, block tridiagonal over the knots: the grid-wide solver eliminates it from both ends towards the middle
 * knot (two chains), and the factorisation is ~85 % of a 256-agent mission.  After this call the session is rank `rank` of a pair of
 * identical sessions (same missions, same options, one per GPU / process): rank 0 eliminates and substitutes along the lower chain, rank 1
 * along the upper one, both assemble the middle knot; row sweeps, control and polish are replicated and bit-identical, so both ranks
 * end with the SAME bits as an unsharded run.  Three kinds of exchange per interior-point iteration go through the caller's hook
 * (the library owns send_dev / recv_dev, in HBM; the session's stream is synchronised before the hook is called; the hook returns 0 once the
 * peer's `bytes` are in recv_dev, e.g. an all-gather over RCCL / xGMI -- swarm_simulator_amd/sharded.py): the explicit inverse of each
 * chain's last knot (81 N^2 doubles rounded up to 64-wide tiles: 42 MB at 256 agents), and two vectors per Newton solve.  The hook is
 * called on the thread that calls rbp_session_run; rbp_session_run_async is refused for a sharded session.  nranks must be 2 (1 = undo).
 * KEEPING THE RANKS MATCHED.  Only the replicated state keeps the two ranks' exchanges paired, so every exchange begins with a 64-byte
 * header (sequence number, kind, byte count, a hash of the state words the rank polled last, a poison word) that each rank compares with
 * its own after the hook has returned: ranks that have diverged -- or a peer that failed on its side and sent the poison word in place of
 * its next exchange -- end the run with RBP_ERR_EXCHANGE and a message naming the word, instead of a hang or a payload unpacked into the
 * wrong slot.  A hook that fails (non-zero return) ends the run with RBP_ERR_EXCHANGE on that rank; the peer is then blocked in ITS hook, so
 * a hook must not wait for ever: rbp_rccl_exchange (include/rbp_rccl.h) polls with a timeout and aborts its communicator, which releases the
 * peer.  After RBP_ERR_EXCHANGE on either rank BOTH ranks must give the solve up (undo the sharding, make a new pair). */
typedef int (*rbp_exchange_fn)(void* user, void* send_dev, void* recv_dev, size_t bytes);
int rbp_session_shard_joint(rbp_session* s, int32_t rank, int32_t nranks, rbp_exchange_fn exchange, void* user);
/* The same with a STREAM-ORDERED exchange (round 6): the hook only ENQUEUES the exchange of `bytes` bytes on `stream` (a hipStream_t: the stream the
 * run was given) and returns -- ncclSend + ncclRecv in one group on that stream (rbp_rccl_exchange_stream of include/rbp_rccl.h) --, and the library
 * synchronises for no exchange: it packs, writes the header, calls the hook, and enqueues the kernel that compares the peer's header with its own and
 * the kernel that unpacks (which does nothing once a header has not matched); the comparison's verdict is read with the once-per-round poll of the
 * missions' states, and a mismatch ends the run with RBP_ERR_EXCHANGE as above.  ~900 host synchronisations of a 256-agent solve become ~100.
 * A peer that is gone leaves the stream blocked in its receive: the per-round wait therefore polls with a clock, and after `timeout_s` seconds
 * (<= 0: for ever) calls `abort_peer(user)` -- may be NULL; rbp_rccl_abort aborts the communicator, which releases both ranks -- and returns
 * RBP_ERR_EXCHANGE.  Everything else as rbp_session_shard_joint (which it replaces on the session; nranks = 1 undoes either). */
typedef int (*rbp_exchange_stream_fn)(void* user, void* send_dev, void* recv_dev, size_t bytes, void* stream);
typedef int (*rbp_exchange_abort_fn)(void* user);
int rbp_session_shard_joint_stream(rbp_session* s, int32_t rank, int32_t nranks, rbp_exchange_stream_fn exchange, rbp_exchange_abort_fn abort_peer,
                                   void* user, double timeout_s);
/* solver options of this session (default: the context's, else rbp_solver_opts_defaults).  The QP workspace is reserved by the first
 * PLANNER run, for the options then in force: a session that only runs the CORRIDOR stage reserves none. */
int rbp_session_set_solver_opts(rbp_session* s, const rbp_solver_opts* o);
/* restrict the CORRIDOR stage of later `run` calls to agents / pair rows [agent_begin, agent_end) (see
 * rbp_corridor_update_range); [0, N) restores the whole mission */
int rbp_session_set_agent_range(rbp_session* s, int32_t agent_begin, int32_t agent_end);
/* blocks on `stream`, copies outputs into plans[0..K-1]; returns the first non-zero per-mission status
 * and, if `status` != NULL, every mission's status in status[0..K-1]. */
int rbp_session_download(rbp_session* s, rbp_plan* plans, int32_t* status, void* stream);
/* clears the per-run status / diagnostics so that `run` can be repeated (bench loops).  T, the SFC end times and the RSFC
 * times are never rescaled on the device -- rbp_session_download applies time_scale to the host copies (rbp_planner.hpp:
 * 250-264) -- so nothing else has to be restored; corridor inputs handed to rbp_session_create are uploaded again in case
 * a CORRIDOR stage overwrote them. */
int rbp_session_reset(rbp_session* s, void* stream);
void rbp_session_destroy(rbp_session* s);

/* Device views of one mission's corridor arrays inside a session (HIP device pointers into the session's arena, valid until
 * rbp_session_destroy): what an agent-sharded Corridor::update exchanges between GPUs WITHOUT a host round trip --
 * the shard written by a CORRIDOR run restricted with rbp_session_set_agent_range is gathered from / into these arrays on the
 * device (swarm_simulator_amd/sharded.py: torch tensors over the pointers, one all_gather_into_tensor over RCCL), and the PLANNER stage
 * of the same session then runs on the completed corridor.  Layouts are those of rbp_plan with the session's strides:
 * sfc_box [N][max_boxes][6] f64, sfc_time [N][max_boxes] f64, sfc_count [N] i32, rsfc_normal [npair][M][3] f32, rsfc_time [M] f64. */
typedef struct rbp_device_arrays {
    void* sfc_count;
    void* sfc_box;
    void* sfc_time;
    void* rsfc_normal;
    void* rsfc_time;
    void* status;                   /* [1] i32: the mission's first error so far (0 = ok), written by the kernels */
    int32_t N, M, max_boxes, npair; /* M, max_boxes: the strides of the arrays (the session's maxima) */
    int32_t device;
} rbp_device_arrays;
int rbp_session_device_arrays(rbp_session* s, int32_t mission, rbp_device_arrays* out);

/* work counters of the last `run`, for the roofline report: see DESIGN.md */
typedef struct rbp_counters {
    double sfc_samples;     /* getDistance-equivalent samples tested by the SFC kernel (summed over missions) */
    double qp_flops;        /* flops of the dense block factorisations/solves the QP kernel executed (grid-wide joint solver: the
                               ALGORITHMIC figure of the mission -- tile sweeps + substitutions -- whether or not panel rows are re-formed
                               per tile, and on each rank of a pair that shares the solve) */
    double qp_ipm_iters;    /* interior-point iterations summed over QPs */
    double qp_solves;       /* number of batch QPs solved */
    double qp_constraint_rows; /* inequality rows swept (rows x passes) */
    double qp_polished;     /* batch QPs whose active-set polish was accepted (the rest keep the interior-point answer) */
    double qp_row_bytes;    /* algorithmic HBM bytes the QP kernel moves (row state and constants per sweep, knot blocks per
                               factorisation / substitution): the numerator of the HBM-side roofline, DESIGN.md 3.3 */
    double kkt_max;         /* max of rbp_plan::kkt_max over the missions */
} rbp_counters;
int rbp_session_counters(rbp_session* s, rbp_counters* out, void* stream);

/* bytes of QP workspace one mission of this session occupies (0 until it has been reserved) */
size_t rbp_session_workspace_bytes(rbp_session* s);
/* reserve (and clear) the QP workspace for the solver options in force now, instead of leaving it to the first PLANNER run: a caller that
 * times its first plan, or wants the allocation failure before it has uploaded anything else */
int rbp_session_reserve_workspace(rbp_session* s, void* stream);

/* raw per-mission diagnostic scalars of the last run: out[K][n], n <= 36 = SC_N (layout: kernels/rbp_dev.h SC_*) */
int rbp_session_scalars(rbp_session* s, double* out, int n, void* stream);

/* ---- contexts: device memory kept across calls -------------------------------------------------
 * "device selection passed through an opaque context handle created once".  A context owns one device
 * arena that the synchronous calls below (and sessions created in it) reuse, so a caller that plans repeatedly -- the
 * reference's ROS node, one Corridor::update + RBPPlanner::update per plan -- pays hipMalloc/hipFree once, not per call.
 * rbp_corridor_update / rbp_planner_update (no context argument) use a per-thread default context on the calling thread's
 * current device.  device < 0 = the calling thread's current device.  One live session per context at a time. */
typedef struct rbp_ctx rbp_ctx;
int rbp_ctx_create(rbp_ctx** out, int device);
/* options of every later session / one-shot call in this context; ctx == NULL: the calling thread's default context (created on the
 * calling thread's current device if it does not exist yet) */
int rbp_ctx_set_solver_opts(rbp_ctx* ctx, const rbp_solver_opts* o);
void rbp_ctx_destroy(rbp_ctx* ctx);
int rbp_ctx_corridor_update(rbp_ctx* ctx, const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan);
int rbp_ctx_planner_update(rbp_ctx* ctx, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan);
/* Corridor::update && RBPPlanner::update in one call (one upload, one download): what swarm_traj_planner_rbp.cpp:96-116 does
 * back to back.  Returns the first failing stage's code. */
int rbp_ctx_plan_update(rbp_ctx* ctx, const rbp_world* world, const rbp_mission* mission, const rbp_param* param, rbp_plan* plan);
/* a batched session whose device memory is the context's arena (released back to it by rbp_session_destroy) */
int rbp_session_create_in(rbp_ctx* ctx, rbp_session** out, int K, const rbp_world* worlds, const rbp_mission* missions,
                          const rbp_param* param, const rbp_plan* plans);

/* the calling thread's default context (see above) is released when the thread exits; a long-lived thread that is done planning
 * can give the arena back earlier */
void rbp_release_thread_context(void);

/* library/version/diagnostics.  RBP_ABI_VERSION changes whenever a struct of this header changes its layout; a binding built
 * against another header must refuse to run (rbp_plan / rbp_counters are written by the library).  rbp_sizeof lets a binding
 * that cannot see this header (ctypes, cgo) compare its own struct sizes with the library's. */
#define RBP_ABI_VERSION 6  /* 1: round 1; 2: rbp_plan.qp_solves/qp_unpolished/kkt_max, rbp_counters.qp_row_bytes/kkt_max; 3: contexts, device views;
                              4: rbp_solver_opts (the library no longer reads environment variables); 5: rbp_session_shard_joint, RBP_ERR_EXCHANGE;
                              6: rbp_param.timescale_rule, rbp_plan.time_scale_alt */
enum { RBP_SIZEOF_WORLD = 0, RBP_SIZEOF_MISSION = 1, RBP_SIZEOF_PARAM = 2, RBP_SIZEOF_PLAN = 3, RBP_SIZEOF_COUNTERS = 4, RBP_SIZEOF_DEVICE_ARRAYS = 5,
       RBP_SIZEOF_SOLVER_OPTS = 6, RBP_SIZEOF_ECBS_OUT = 7, RBP_SIZEOF_REPORT = 8, RBP_SIZEOF_DYNAMICS = 9, RBP_SIZEOF_CLEARANCE = 10, RBP_SIZEOF_SEPARATION = 11,
       RBP_SIZEOF_SWEPT_CLEARANCE = 12, RBP_SIZEOF_LIMITS = 13, RBP_SIZEOF_SESSION_CAPACITY = 14 };
int rbp_abi_version(void);
size_t rbp_sizeof(int which);
const char* rbp_version(void);
/* ---- distance grid of a world on the GPU ---------------------------------
 * What  DynamicEDTOctomap distmap(max_dist, tree, bbx_min, bbx_max, false); distmap.update();  followed by getDistance() on every
 * voxel centre of the box yields (swarm_traj_planner_rbp_test_all.cpp:57-63, swarm_traj_planner_rbp.cpp:73-80): the float grid
 * rbp_world.dist points at, [nx][ny][nz] with z fastest, clamped at ((int)(max_dist / res + 1)) cells like dynamicEDT3D.
 * leaf_keys: [n_leaves][4] = min-corner voxel key minus 32768 (x, y, z) and edge length in voxels of every occupied leaf (what
 * rbp_octomap_load_bt of rbp_host.h returns).  rbp_edt_dims gives the grid shape (dim, key_min as in rbp_world) for a box;
 * rbp_edt_build fills dist (host buffer of dim[0]*dim[1]*dim[2] floats): a set of one world (rbp_dev_worlds, below) copied back.
 * Bit-identical to the host library's rbp_world_build. */
int rbp_edt_dims(double res, const double bbx_min[3], const double bbx_max[3], int32_t dim[3], int32_t key_min[3]);
int rbp_edt_build(const int32_t* leaf_keys, int64_t n_leaves, double res, const double bbx_min[3], const double bbx_max[3],
                  double max_dist, float* dist);

/* ---- worlds that stay on the device -------------------------------------------------------------
 * One build for a SET of W worlds (the 50 maps of swarm_traj_planner_rbp_test_all.cpp:49-103): the number of kernel launches does not
 * depend on W, the W float grids lie in one device allocation owned by the set, and nothing returns to the host.  leaf_keys[w] /
 * n_leaves[w]: the occupied leaves of world w as for rbp_edt_build (leaf_keys[w] may be NULL where n_leaves[w] is 0); res[w]: its
 * resolution, which with the common box gives every world its own shape by rbp_edt_dims' rule; one max_dist for all.  Every grid is
 * bit-identical to what rbp_edt_build / rbp_world_build give for that world.  Argument errors (null out, W <= 0, negative n_leaves,
 * bbx_max < bbx_min, res <= 0, max_dist <= 0) are RBP_ERR_BAD_ARGUMENT before a device is looked for. */
typedef struct rbp_dev_worlds rbp_dev_worlds;
/* builds W grids on `device` (< 0: current) and returns when they are complete */
int  rbp_dev_worlds_create(rbp_dev_worlds** out, int device, int32_t W, const int32_t* const* leaf_keys, const int64_t* n_leaves,
                           const double* res /* [W] */, const double bbx_min[3], const double bbx_max[3], double max_dist);
int  rbp_dev_worlds_count(const rbp_dev_worlds* ws);
/* fills dim / key_min / res; out->dist is a DEVICE pointer, valid until destroy */
int  rbp_dev_worlds_get(const rbp_dev_worlds* ws, int32_t w, rbp_world* out);
int  rbp_dev_worlds_download(const rbp_dev_worlds* ws, int32_t w, float* dist_host);
void rbp_dev_worlds_destroy(rbp_dev_worlds* ws);
/* The coarse obstacle mask of the ECBS front-end (ECBSPlanner::setObstacles, ecbs_planner.hpp:80-109) from the resident grid of world w:
 * what rbp_ecbs_obstacles of rbp_host.h computes from a host grid, same arguments and return values (0; 1: a sample of the planning
 * lattice lies outside the grid; obstacle_host == NULL only fills dim), to be handed to rbp_ecbs_plan_obstacles.  One thread per sample
 * looks the distance up; dim[0] * dim[1] * dim[2] bytes come back instead of the grid. */
int  rbp_dev_worlds_ecbs_obstacles(const rbp_dev_worlds* ws, int32_t w, const rbp_mission* mission, const rbp_param* param, int32_t dim[3],
                                   uint8_t* obstacle_host, size_t capacity);

/* ---- the ECBS front-end search on the device --------------------------------
 * The search of rbp_ecbs_plan_obstacles (rbp_host.h; csrc/host/ecbs.cpp) for K missions in one call, one wavefront per mission
 * (kernels/ecbs.hip).  It is the host library's own deterministic search, so for a mission that ends with status 0, 1 or 2 every output
 * equals what rbp_ecbs_plan_obstacles / rbp_ecbs_plan return for the same mask, mission, param and budget: init_traj and T bit for bit,
 * M, makespan, sum_cost and both expansion counters.  Missions with a status other than 0 get zeros in their outputs.
 * Status 3 (RBP_ECBS_CAPACITY) has no host counterpart: the mission exceeded a capacity of the device search -- a path longer than
 * max_M - 2 steps in any high-level node, 32768 nodes of one low-level search -- and the library does NOT fall back to the CPU; the
 * caller decides (rbp_ecbs_plan_obstacles, or a larger max_M).
 * The return value is RBP_OK when the call itself worked; per-mission outcomes are in `status`.  Argument errors are
 * RBP_ERR_BAD_ARGUMENT before a device is looked for: a null pointer, K <= 0, missions of differing N, N outside 1..256, a planning
 * lattice with more than 1024 cells on an axis (or whose seen bitmap, cells x (8 (dimx + dimy + dimz) + 64 + max_M) bits, exceeds
 * 16 MB), max_M outside 2..4096, max_high_level_nodes outside 1..RBP_ECBS_MAX_HIGH_LEVEL_NODES (B budgeted expansions need 2 B + 1
 * node slots), a dim that is not param's lattice, a world index outside the set.  ecbs_w < 1 leaves the focal sets empty: status 2. */
enum { RBP_ECBS_CAPACITY = 3, RBP_ECBS_MAX_HIGH_LEVEL_NODES = 512 };
typedef struct rbp_ecbs_out {       /* caller-owned; all missions of a call share N */
    int32_t  max_M;                 /* capacity in segments (makespan + 2 must fit) */
    int32_t* status;                /* [K] 0 ok; 1 start/goal occluded or lattice sample outside the grid;
                                       2 search failed / high-level budget exhausted (the host's codes);
                                       3 RBP_ECBS_CAPACITY: a device capacity (max_M, node pool) was exceeded */
    int32_t* M; int32_t* makespan; int32_t* sum_cost;         /* [K] */
    int64_t* high_level_expanded; int64_t* low_level_expanded; /* [K] */
    double*  T;                     /* [K][max_M+1] */
    float*   init_traj;             /* [K][N][max_M+1][3] */
} rbp_ecbs_out;

/* the search on K obstacle masks of one lattice shape (host pointers, [dimx][dimy][dimz] of 0/1); device < 0: the current one */
int rbp_dev_ecbs_plan_masks(int device, int32_t K, const int32_t dim[3], const uint8_t* const* obstacle,
                            const rbp_mission* missions, const rbp_param* param,
                            int64_t max_high_level_nodes, rbp_ecbs_out* out);
/* the same for missions on resident worlds (mission k on world world_index[k] of the set): masks are made on the device
   (the kernel behind rbp_dev_worlds_ecbs_obstacles, for all K in one launch) and never leave it */
int rbp_dev_worlds_ecbs_plan(const rbp_dev_worlds* ws, int32_t K, const int32_t* world_index,
                             const rbp_mission* missions, const rbp_param* param,
                             int64_t max_high_level_nodes, rbp_ecbs_out* out);

/* ---- the search's plans handed to a session without a host trip --------------------------------
 * rbp_dev_worlds_ecbs_search is the search of rbp_dev_worlds_ecbs_plan -- same argument checks (max_M is an argument here, there is no
 * rbp_ecbs_out to fill), same refusals with RBP_ERR_BAD_ARGUMENT before a device is looked for, same capacities, same statuses 0 / 1 /
 * 2 / 3 -- whose results STAY in HBM, owned by the handle: per mission the status, the path lengths, the packed paths, both expansion
 * counters, and the missions' start, goal, radius, max_vel and max_acc, COPIED once as packed arrays [K][N][...] (the caller's mission
 * arrays are not needed after the call; max_vel / max_acc may be null for a search that is only downloaded).  Only status, lengths
 * and counters return to the host, K x (N + 3) words.  The handle REFERENCES the set of worlds: `ws` must outlive it.
 * rbp_dev_ecbs_download fills a caller's rbp_ecbs_out (out->max_M must be the search's) with exactly what rbp_dev_worlds_ecbs_plan returns
 * for the same arguments, bit for bit, the zeros beyond index M and of missions without a result included.  out->T and out->init_traj
 * may be NULL: then only the per-mission scalars are filled and nothing is computed; otherwise both are written on the device
 * (kernels/handoff.hip) and copied back once. */
typedef struct rbp_dev_ecbs rbp_dev_ecbs;
int  rbp_dev_worlds_ecbs_search(const rbp_dev_worlds* ws, int32_t K, const int32_t* world_index, const rbp_mission* missions,
                                const rbp_param* param, int64_t max_high_level_nodes, int32_t max_M, rbp_dev_ecbs** out);
int  rbp_dev_ecbs_count(const rbp_dev_ecbs* e);   /* K of the search (0 for a null handle) */
int  rbp_dev_ecbs_download(const rbp_dev_ecbs* e, rbp_ecbs_out* out);
void rbp_dev_ecbs_destroy(rbp_dev_ecbs* e);
/* A session of the missions of `e` whose status is 0, in ascending order, on the device of the search: slot_of[k] (slot_of may be NULL;
 * [rbp_dev_ecbs_count(e)]) receives mission k's index in the session, or -1.  No mission with status 0: RBP_ERR_BAD_ARGUMENT.  Every
 * mission keeps its own M; max_boxes <= 0 means each mission's M.  T, init_traj and the five mission arrays are written into the session's
 * arena by two kernels from what the handle holds: nothing of them passes through the host, everything is COPIED, and the handle may be
 * destroyed as soon as the call has returned.  The worlds are the resident grids of the handle's set, REFERENCED in place like any device
 * grid of rbp_world: the set of worlds must outlive the session.  T is the search's (i * time_step of the param the SEARCH was given);
 * `param` here is the plan's, and keeping the two consistent is the caller's business.  The session has no corridor inputs; run,
 * run_async, download, reset, device_arrays, set_solver_opts ... work as on a session of rbp_session_create.  A search whose missions
 * came without max_vel / max_acc is refused. */
int  rbp_session_create_from_ecbs(rbp_session** out, const rbp_dev_ecbs* e, const rbp_param* param, int32_t max_boxes, int32_t* slot_of);

/* ---- a session that outlives its missions: refilled from the next search, allocating nothing ---------
 * A session's CAPACITY is what its arena was laid out for: K missions of N agents, slots of M segments and max_boxes boxes per agent.
 * rbp_session_capacity_of returns it for every session: the K, N and the largest M / max_boxes a session of rbp_session_create,
 * rbp_session_create_in or rbp_session_create_from_ecbs was created with, or what rbp_session_create_reserved was given.
 * rbp_session_create_reserved builds an EMPTY session of that capacity on the device of `ws`, whose grids it will reference in place
 *   (the set must outlive the session): the arena, the pinned staging block of the refills (K source indices, K M, K max_boxes and K
 *   world descriptors, with its device twin and an event) and nothing else; the QP workspace and the reports' buffers are reserved by the
 *   first call that needs them, as in every session, for the CAPACITY, and kept across refills.  Until it has been refilled the session
 *   holds no mission: run, run_async, download and the reports are RBP_ERR_BAD_ARGUMENT ("holds no mission").  Null out / ws / cap / param,
 *   K or N < 1, M < 2, max_boxes < 1 and the refusals of rbp_param known from rbp_session_create are RBP_ERR_BAD_ARGUMENT before a device
 *   is looked for.
 * rbp_session_refill_from_ecbs replaces the session's missions by those of `e` whose status is 0: they become slots 0 .. K'-1 in ascending
 *   order, every mission keeps its own M, max_boxes <= 0 means each mission's M, and slot_of is written as by
 *   rbp_session_create_from_ecbs.  The slot strides stay the capacity's; only the number of missions and their M / max_boxes change.  The
 *   session is then as a fresh session of those missions: status, scalars and counters are cleared, it has no corridor inputs, and the
 *   reports refuse until the next PLANNER run, after which every output has the bits a session of rbp_session_create_from_ecbs gives.
 *   The call ALLOCATES NOTHING and frees nothing: source list, M, max_boxes and the K' world descriptors go up in ONE asynchronous copy
 *   of the session's pinned staging block, one kernel (kernels/handoff.hip session_refill_kernel) on `stream` writes T, init_traj and the
 *   mission arrays from what the handle holds and clears what a run reads or a download hands out of the slots' previous missions, and one
 *   asynchronous clear on `stream` covers the K' blocks of the QP workspace if one has been reserved.  Everything is COPIED: the handle
 *   may be destroyed as soon as the kernel has run (after a synchronisation of `stream`).  The call first joins an asynchronous solve, like
 *   every session call, and it does NOT synchronise, with one exception: the staging block is reused, so a refill waits on the event
 *   recorded behind the PREVIOUS refill's copy -- which has long completed when a run lies between the two.  The refill must be enqueued
 *   on the stream the session's runs use, or ordered after them by the caller.  A session that was not created reserved reserves its
 *   staging block in its first refill; it is refillable when all its grids are grids of the handle's set of worlds.
 *   RBP_ERR_BAD_ARGUMENT, with the session left exactly as it was: a null session or handle (before a device is looked for); a handle on
 *   another device or another set of worlds than the session's; e's N differs from the session's; no mission with status 0, or more than
 *   the capacity's K; a mission's M or box capacity above the strides; a search whose missions came without max_vel / max_acc; a session
 *   sharded over two ranks (rbp_session_shard_joint*); a session whose asynchronous solve failed (that error is returned). */
typedef struct rbp_session_capacity { int32_t K, N, M, max_boxes; } rbp_session_capacity;
int  rbp_session_create_reserved(rbp_session** out, const rbp_dev_worlds* ws, const rbp_session_capacity* cap, const rbp_param* param);
int  rbp_session_capacity_of(const rbp_session* s, rbp_session_capacity* out);
int  rbp_session_refill_from_ecbs(rbp_session* s, const rbp_dev_ecbs* e, int32_t max_boxes, int32_t* slot_of, void* stream);

/* ---- ... refilled from a caller's own plans, staged in one copy -------------------------------------------
 * The other source of a refill: host rbp_plans from any front-end, with their missions and worlds, as rbp_session_create takes them.
 * rbp_session_refill_from_plans replaces the session's missions by the K given ones, which become slots 0 .. K-1.  It reads
 *   plans[k].{N, M, max_boxes, T, init_traj}, all five arrays of missions[k] and worlds[k]; corridor arrays in a plan are ignored, and the
 *   session has no corridor inputs afterwards, as after the other refill.  worlds[k].dist must be a DEVICE pointer on the session's device
 *   -- a grid of a rbp_dev_worlds or any device allocation of that layout -- which is referenced in place and stays the caller's until
 *   the next refill or the session's end; a host grid is refused, a refill uploads no grid.  The session is then as a fresh session of
 *   rbp_session_create of those missions: after a run every output has that session's bits.
 *   The host packs the missions tightly into a pinned staging block, as many consecutive missions as fit (per mission M, max_boxes, the
 *   world descriptor, T, init_traj and the 25 N doubles of the mission arrays); ONE asynchronous copy per round sends the block up and ONE
 *   kernel (kernels/handoff.hip session_refill_plans_kernel) on `stream` writes the round's slots and clears what
 *   rbp_session_refill_from_ecbs clears.  A batch that does not fit the block goes in several rounds on `stream`; the host waits only on
 *   the event behind the previous copy out of the block before it packs the next round -- for a one-round refill that is the previous
 *   refill's copy.  After the last round one asynchronous clear covers the K blocks of the QP workspace if one has been reserved.
 *   Nothing is allocated once the block exists, and nothing else synchronises.  The host arrays may be released on return (they are
 *   copied into the block); the stream rule of rbp_session_refill_from_ecbs holds.  A session of any constructor is refillable within its
 *   own capacity.
 *   RBP_ERR_BAD_ARGUMENT, with a message that names the mission and the field and the session left exactly as it was: a null session,
 *   K < 1, null worlds / missions / plans (before a device is looked for); a sharded session; K above the capacity's; a plan's or
 *   mission's N other than the capacity's; M outside [2, capacity M]; max_boxes outside [1, capacity max_boxes]; a null T, init_traj,
 *   start, goal, radius, max_vel, max_acc or dist; a grid that is not device memory of the session's device; grids whose occupancy mask
 *   needs more LDS than the device has (as rbp_session_refill_from_ecbs checks it).
 * rbp_plan_stage_bytes is a pure function (it looks for no device): the bytes K missions of the capacity's shape (N, M) occupy in the
 *   staging block.  A mission of a smaller M occupies less.  A null or non-positive capacity, K < 1 or null bytes: RBP_ERR_BAD_ARGUMENT.
 * rbp_session_reserve_plan_stage reserves the pinned block, its device twin and its event with `bytes` of room;
 *   0 means min(rbp_plan_stage_bytes(capacity, capacity K), RBP_REFILL_STAGE_BYTES).  Less than one mission of the capacity's shape, or a
 *   second call with another size, is RBP_ERR_BAD_ARGUMENT and leaves the block as it is.  The call is optional: the first
 *   rbp_session_refill_from_plans makes it with 0 itself; a caller who reserves up front pays no allocation even in the first refill. */
#define RBP_REFILL_STAGE_BYTES (64u << 20)
int  rbp_plan_stage_bytes(const rbp_session_capacity* cap, int32_t K, size_t* bytes);
int  rbp_session_reserve_plan_stage(rbp_session* s, size_t bytes);
int  rbp_session_refill_from_plans(rbp_session* s, int32_t K, const rbp_world* worlds, const rbp_mission* missions,
                                   const rbp_plan* plans, void* stream);

/* ---- a mission's acceptance signals on the device ---------------------------
 * The two numbers the reference prints per plan (rbp_publisher.hpp:685-695, 769-798): the smallest safety ratio -- downwash-scaled
 * distance of two agents over the sum of their radii, should be >= 1 -- over all pairs at every sample t = j * dt, j < floor(T[M] / dt),
 * and the summed length of the agents' sampled paths.  The arithmetic is stated once, in csrc/common/report_rules.h, for the kernels
 * (kernels/report.hip) and for rbp_report_host of rbp_host.h: both return the same bits.  They are not the bits of rbp_validate, whose
 * std::pow polynomial and single running sum no GPU reproduces: positions are Horner's scheme here, the distance is a sum per agent and
 * then over the agents, and the minimum names the lexicographically first (sample, qi, qj) among equal ratios; a NaN is never the minimum.
 * rbp_session_report: the reports of a session's K missions from its own coef, T, time scale, radius and status, which stay in HBM: it
 *   waits for an asynchronous solve like every call, enqueues two kernels on `stream`, copies K structs back in one copy and returns when
 *   they have arrived.  Nothing of the session changes.  A mission whose status is not 0 is reported with that status and nothing else.
 *   RBP_ERR_BAD_ARGUMENT: a session whose last run did not include the PLANNER stage; more agents than one sample's positions fit the LDS
 *   budget for (1365); and, before a device is looked for, a null pointer or dt <= 0.
 * rbp_dev_report: the same kernels on a caller's host arrays, uploaded once -- coefficients from anywhere, the reference's own log for one.
 *   Mission k has M[k] <= M_stride segments; T is [K][M_stride + 1] (M[k] + 1 entries used), not scaled; time_scale [K] multiplies it as
 *   rbp_session_download does (NULL: 1); coef holds per mission a slot of N * 3 * 6 * M_stride doubles with the mission's own
 *   [N][3][6 M[k]] at its front, a session's layout; radius [K][N].  device < 0: the current one.  Argument errors (a null pointer,
 *   K, N <= 0, an M[k] outside 1..M_stride, dt, downwash or a time scale <= 0) are RBP_ERR_BAD_ARGUMENT before a device is looked for. */
#define RBP_REPORT_MAX_SAMPLES (1 << 20)
typedef struct rbp_report {
    double  min_safety_ratio;      /* 1e9: no pair or no sample */
    double  total_flight_distance;
    double  end_time;              /* Ts[M]: the mission's last segment time, scaled */
    int32_t samples;               /* -1: more than RBP_REPORT_MAX_SAMPLES, nothing else computed (ratio 1e9, distance 0) */
    int32_t min_sample, min_qi, min_qj;  /* where the minimum is; -1: none */
    int32_t status;                /* the mission's status; != 0: nothing computed, ratio 0, distance 0, end time 0, no samples, indices -1 */
    int32_t reserved;
} rbp_report;
int rbp_session_report(rbp_session* s, double dt, rbp_report* out /* [K] */, void* stream);
int rbp_dev_report(int device, int32_t K, int32_t N, const int32_t* M /* [K] */, int32_t M_stride,
                   const double* T /* [K][M_stride+1], unscaled */, const double* time_scale /* [K] or NULL = 1 */,
                   const double* coef /* per mission the session's layout */, const double* radius /* [K][N] */,
                   double downwash, double dt, rbp_report* out /* [K] */);

/* ---- the sampled states of resident plans, their limit peaks and ratio curves (the rest of it) ----
 * What the reference's publisher samples of a plan at t = j * dt, j < samples, besides the two numbers above (rbp_publisher.hpp:670-683
 * update_quad_state, 697-767 plot_quad_dynamics, 769-798 update_safety_margin_ratio), by the rule of csrc/common/state_rules.h, which
 * the kernels (kernels/dynamics.hip) and rbp_dynamics_host of rbp_host.h share: both return the same bits.  Times, samples, the segment of
 * a sample and positions are the report's (report_rules.h).
 *   states  [K][N][9][S_stride]: agent, row, sample; row / 3 = derivative (position, velocity, acceleration), row % 3 = axis.  Velocity
 *           and acceleration are Horner's scheme over the differentiated coefficients, every product and sum rounded on its own.
 *   curves  [K][S_stride][2]: per sample the smallest (from 1e9) and the largest (from 0) safety ratio over the pairs; a NaN moves neither.
 *   peaks   the largest |v_k| / max_vel[agent][k] and |a_k| / max_acc[agent][k] over samples, agents and axes -- above 1 the plan breaks a
 *           limit at a sample, which the literal timeScale rule (rbp_param.timescale_rule) can leave behind -- each with the value itself
 *           (signed), the limit it was divided by, and the lexicographically first (sample, agent, axis) among equal ratios; a ratio
 *           that is 0, negative or NaN is never a peak.
 * states and curves may each be NULL, a host pointer, or a device pointer on the plans' device (classified with hipPointerGetAttributes as
 * rbp_world.dist is; another device: RBP_ERR_BAD_ARGUMENT).  A device destination is written in place by the kernels.  A host destination
 * goes through a staging allocation of at most RBP_DYNAMICS_STAGE_BYTES (one mission's rows where those alone are larger), a chunk of
 * missions at a time.  A mission with samples > S_stride or samples = -1 has nothing stored and stored = 0 (its peaks are still reported,
 * except for -1); entries beyond a mission's `samples` are left untouched, as is everything of a mission that is not stored.  Size the
 * buffers from rbp_session_report's `samples`.  S_stride is not read where both are NULL.
 * rbp_session_dynamics: of a session's K missions, from its own arrays, which stay in HBM; waits for an asynchronous solve, refuses a
 *   session whose last run had no PLANNER stage and more than 1365 agents, and checks its arguments before a device is looked for (a null
 *   session or `out`, dt <= 0, S_stride < 1 with a buffer), all as rbp_session_report does.  A mission whose status is not 0 gets that
 *   status, nothing computed (zeros, indices -1) and nothing stored.  Nothing of the session changes.
 * rbp_dev_dynamics: the same kernels on a caller's host arrays in rbp_dev_report's layout, with max_vel / max_acc [K][N][3]. */
#define RBP_DYNAMICS_STAGE_BYTES (64 << 20)
typedef struct rbp_dynamics {
    double  peak_vel_ratio, peak_vel, peak_vel_limit;   /* 0: no sample */
    double  peak_acc_ratio, peak_acc, peak_acc_limit;
    double  end_time;
    int32_t samples;                                    /* as rbp_report.samples, -1 included */
    int32_t vel_sample, vel_agent, vel_axis;            /* -1: none */
    int32_t acc_sample, acc_agent, acc_axis;
    int32_t stored;                                     /* 1: states / curves of this mission were written */
    int32_t status;
} rbp_dynamics;
int rbp_session_dynamics(rbp_session* s, double dt, rbp_dynamics* out /* [K] */,
                         double* states /* [K][N][9][S_stride] or NULL */,
                         double* curves /* [K][S_stride][2] or NULL */,
                         int32_t S_stride, void* stream);
int rbp_dev_dynamics(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride,
                     const double* T, const double* time_scale, const double* coef,
                     const double* radius, const double* max_vel, const double* max_acc,
                     double downwash, double dt, rbp_dynamics* out,
                     double* states, double* curves, int32_t S_stride);

/* ---- the clearance of resident plans to the obstacles (does the plan hit anything, and where is it closest) ----
 * The distance grid's value under every agent at every sample t = j * dt, j < samples, less the agent's radius, by the rule of
 * csrc/common/clearance_rules.h, which the kernels (kernels/clearance.hip) and rbp_clearance_host of rbp_host.h share: both return the same
 * bits.  Times, samples, the segment of a sample and positions are the report's (report_rules.h).  The lookup is
 * DynamicEDTOctomap::getDistance(point3d) as rbp_world describes it: the coordinate rounded to float, the key floor((1 / res) * (double)pf),
 * -1 outside the grid.  A (sample, agent) item is a HIT where the grid reads less than radius - 1e-6 (rbp_corridor.hpp:67, SP_EPSILON_FLOAT)
 * and an OUTSIDE where its lookup left the grid (also a hit for every radius above -1 + 1e-6, as in the reference).  The minimum names the
 * lexicographically first (sample, agent) among equal clearances; a NaN clearance (a NaN radius) is never the minimum.
 * agent_clearance [K][N] (NULL: not wanted): agent a's smallest clearance over its samples, 1e9 where it has none; the row of a mission that
 * is not computed (a status, or samples = -1) is left untouched.  It may be a host pointer or a device pointer on the plans' device
 * (classified with hipPointerGetAttributes as rbp_world.dist is; another device: RBP_ERR_BAD_ARGUMENT): a device destination is written in
 * place by the kernels, a host destination goes through one staging buffer and one copy.
 * rbp_session_clearance: of a session's K missions, from its own coef, T, time scale, radius and status and the grid of each mission's
 *   world, all of which stay in HBM; waits for an asynchronous solve like every call, enqueues two kernels on `stream`, copies K structs
 *   back in one copy and returns when they have arrived.  Nothing of the session changes.  A mission whose status is not 0 gets that status
 *   and nothing computed.  RBP_ERR_BAD_ARGUMENT: a session whose last run did not include the PLANNER stage; and, before a device is looked
 *   for, a null pointer or dt <= 0 -- as rbp_session_report.  (A session cannot exist without a grid for every mission: rbp_session_create
 *   refuses a world without one, and rbp_session_create_from_ecbs takes the resident grids of the search's set.)
 * rbp_dev_clearance: the same kernels on a caller's host arrays in rbp_dev_report's layout, uploaded once, and K worlds.  worlds[k].dist
 *   may be a host grid, uploaded once per distinct (pointer, shape), or a device grid on `device`, referenced in place (another device:
 *   RBP_ERR_BAD_ARGUMENT).  Argument errors (a null pointer, K, N <= 0, an M[k] outside 1..M_stride, dt, res or a time scale <= 0, a
 *   dim <= 0) are RBP_ERR_BAD_ARGUMENT before a device is looked for. */
typedef struct rbp_clearance {
    double  min_clearance;   /* metres; 1e9: no sample.  Saturates at (grid clamp - radius): the grid is clamped at its maxDist */
    double  min_dist;        /* the grid's value at the minimum (-1: outside); 0 where there is none */
    double  end_time;        /* Ts[M]: the mission's last segment time, scaled */
    int64_t hits, outside;   /* (sample, agent) counts */
    int32_t samples;         /* as rbp_report.samples, -1 included (then nothing else is computed) */
    int32_t min_sample, min_agent;  /* where the minimum is; -1: none */
    int32_t status;          /* the mission's status; != 0: nothing computed, zeros, indices -1 */
} rbp_clearance;
int rbp_session_clearance(rbp_session* s, double dt, rbp_clearance* out /* [K] */,
                          double* agent_clearance /* [K][N] or NULL; host or device pointer */, void* stream);
int rbp_dev_clearance(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T,
                      const double* time_scale, const double* coef, const double* radius,
                      const rbp_world* worlds /* [K]; dist host or device */, double dt,
                      rbp_clearance* out, double* agent_clearance);

/* ---- a certified interval for the smallest safety ratio of resident plans in CONTINUOUS time ----
 * rbp_report, rbp_dynamics and rbp_clearance look at the samples t = j * dt; the relative Bernstein polynomial promises separation at
 * every instant.  For a pair qi < qj and a segment m (an ITEM) the squared downwash-scaled relative distance is a polynomial of degree
 * 10; on a PIECE of the segment its smallest Bernstein coefficient less an error term is a lower bound of it and its first and last
 * coefficient plus that term are upper bounds of its minimum.  Piece p of depth D covers [p / 2^D, (p+1) / 2^D] of the segment.  All
 * of it -- the Bernstein form, the halving, the squared norm, the error term c u S with its derivation, the 3 doubles every ratio is
 * moved outwards for its square root and division, the order of the minima -- is the rule of csrc/common/separation_rules.h, which the
 * kernels (kernels/separation.hip) and rbp_separation_host of rbp_host.h share: both return the same bits.  The promise:
 *     lower_ratio <= the smallest safety ratio of the mission over all pairs at every instant of [0, Ts[M]] <= upper_ratio,
 * for the polynomials the double coefficients define.  lower_ratio >= 1 certifies the plan; upper_ratio < 1 proves a collision.
 * Refinement is fixed: every item is evaluated at depth 0; an item whose lower ratio there is below refine_below is evaluated again on
 * all 2^depth pieces of depth `depth`, which replace its depth-0 bounds.  depth in 0 .. RBP_SEPARATION_MAX_DEPTH; refine_below > 0
 * (1e9, the ratio of no pair, refines everything).  The minima name the lexicographically first (segment, piece, qi, qj) among equal
 * ratios; a NaN is never a minimum.
 * pair_lower [K][N (N-1) / 2] (NULL: not wanted), in the pair order of rbp_plan: a pair's smallest lower ratio over its segments, 1e9
 * where none is a number; the row of a mission with a status is left untouched.  It may be a host pointer or a device pointer on the
 * plans' device (classified with hipPointerGetAttributes as rbp_world.dist is; another device: RBP_ERR_BAD_ARGUMENT): a device
 * destination is written in place by the kernels, a host destination goes through one staging buffer and one copy.
 * Memory: items that are refined go through a work list of one uint32 per item, sized for the worst case (every item), of at most
 * RBP_SEPARATION_LIST_BYTES; missions are processed in chunks where all of them would need more (a single mission always is one chunk,
 * and one of more than 2^32 - 64 items is refused).  No allocation depends on the data.
 * rbp_session_separation: of a session's K missions, from its own coef, T, time scale, radius and status, all of which stay in HBM;
 *   waits for an asynchronous solve like every call, enqueues its kernels on `stream`, copies K structs back in one copy and returns
 *   when they have arrived.  Nothing of the session changes.  A mission whose status is not 0 gets that status and nothing computed.
 *   RBP_ERR_BAD_ARGUMENT: a session whose last run did not include the PLANNER stage; and, before a device is looked for, a null
 *   pointer, a depth outside 0 .. RBP_SEPARATION_MAX_DEPTH, a refine_below that is not a number above 0.
 * rbp_dev_separation: the same kernels on a caller's host arrays in rbp_dev_report's layout, uploaded once.  Argument errors (those
 *   above, K, N <= 0, an M[k] outside 1..M_stride, a time scale or a downwash <= 0) are RBP_ERR_BAD_ARGUMENT before a device is looked for. */
#define RBP_SEPARATION_MAX_DEPTH 8
#define RBP_SEPARATION_LIST_BYTES (64u << 20) /* the work list's budget: 16 Mi items of a chunk of missions */
typedef struct rbp_separation {
    double  lower_ratio, upper_ratio;   /* 1e9: no pair */
    double  end_time;                   /* Ts[M]: the mission's last segment time, scaled */
    int64_t uncertified, colliding, refined;   /* items whose lower ratio is < 1, whose upper ratio is < 1, that went to `depth` */
    int32_t lower_segment, lower_piece, lower_qi, lower_qj;   /* -1: none */
    int32_t upper_segment, upper_piece, upper_qi, upper_qj;
    int32_t lower_depth, upper_depth;   /* depth of the piece the bound came from (0 or `depth`; -1: none) */
    int32_t status, reserved;           /* the mission's status; != 0: nothing computed, zeros, indices -1 */
} rbp_separation;
int rbp_session_separation(rbp_session* s, int32_t depth, double refine_below, rbp_separation* out /* [K] */,
                           double* pair_lower /* [K][N(N-1)/2] or NULL; host or device pointer */, void* stream);
int rbp_dev_separation(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T,
                       const double* time_scale, const double* coef, const double* radius, double downwash,
                       int32_t depth, double refine_below, rbp_separation* out, double* pair_lower);

/* ---- a certified interval for the smallest clearance of resident plans to the obstacles in CONTINUOUS time ----
 * rbp_clearance reads the distance grid under every agent at the samples t = j * dt; between two samples a fast agent crosses many cells.
 * For an agent a and a segment m (an ITEM) every axis of the position is a polynomial of degree 5; a PIECE of the segment (piece p of
 * depth D covers [p / 2^D, (p+1) / 2^D] of it) lies in the box of its Bernstein control points.  The grid's lookup (rbp_world) is monotone
 * per axis, so the keys of the box's corners, each corner moved outwards by a counted rounding term, enclose the key of every point of
 * the piece, and the smallest grid value over that box of cells (d_lo) bounds every reading on the piece from below.  The smaller of
 * the two lookups at the piece's first and last control point (d_up) is a reading on the curve.  A piece whose box leaves the grid is
 * OUTSIDE and one whose box holds more than RBP_SWEPT_MAX_CELLS cells is OVER BUDGET: neither is scanned, and d_lo is -1.  All of it
 * -- the Bernstein form, the halving, the widening e = (20 + 5 D) 2^-53 A with its derivation, the keys, the order of the minima -- is
 * the rule of csrc/common/swept_rules.h, which the kernels (kernels/swept.hip) and rbp_swept_clearance_host of rbp_host.h share: both
 * return the same bits.  The promise, for the polynomials the double coefficients define and a grid whose values are >= -1:
 *     every reading lookup(p_a(t)) - radius_a, at every instant t of [0, Ts[M]], is >= lower_clearance;
 * lower_clearance > -1e-6, that is uncertified == 0, certifies the plan against the reference's own hit test (d < radius - 1e-6).
 * upper_clearance is a reading at a point the rule computed on the curve, within e of it: a witness (hitting > 0 shows a hit there),
 * not a bound on the exact polynomial.  The lookup is a step function of the position, so nothing stronger is claimed.
 * Refinement is fixed: every item is evaluated at depth 0; an item whose depth-0 box is outside or over budget, or whose lower
 * clearance there is not >= refine_below (a NaN goes too), is evaluated again on all 2^depth pieces of depth `depth`, which replace its
 * depth-0 readings and flags.  depth in 0 .. RBP_SWEPT_MAX_DEPTH; refine_below any number (1e9 refines everything; -2 only what is
 * outside or over budget).  The minima name the lexicographically first (segment, piece, agent) among equal clearances -- grid values
 * are quantised and clamped, so ties are common; a NaN, or 1e9 and more, is never a minimum.
 * agent_lower [K][N] (NULL: not wanted): an agent's smallest lower clearance over its segments, 1e9 where none is a number; the row of a
 * mission with a status is left untouched.  It may be a host pointer or a device pointer on the plans' device (classified as
 * rbp_world.dist is; another device: RBP_ERR_BAD_ARGUMENT): a device destination is written in place by the kernels, a host
 * destination goes through one staging buffer and one copy.
 * Memory: items that are refined go through a work list of one uint32 per item, sized for the worst case (every item), of at most
 * RBP_SWEPT_LIST_BYTES; missions are processed in chunks where all of them would need more (a single mission always is one chunk, and
 * one of more than 2^32 - 64 items is refused).  No allocation depends on the data.
 * rbp_session_swept_clearance: of a session's K missions, from its own coef, T, time scale, radius, status and worlds, all of which stay
 *   in HBM; waits for an asynchronous solve like every call, enqueues its kernels on `stream`, copies K structs back in one copy and
 *   returns when they have arrived.  Nothing of the session changes.  A mission whose status is not 0 gets that status and nothing
 *   computed.  RBP_ERR_BAD_ARGUMENT: a session whose last run did not include the PLANNER stage; and, before a device is looked for, a
 *   null pointer, a depth outside 0 .. RBP_SWEPT_MAX_DEPTH, a refine_below that is no number.
 * rbp_dev_swept_clearance: the same kernels on a caller's host arrays in rbp_dev_clearance's layout, uploaded once; worlds[k].dist may be
 *   a host or a device pointer.  Argument errors (those above, K, N <= 0, an M[k] outside 1..M_stride, a time scale <= 0, a world
 *   without a grid, with a res <= 0 or a dim <= 0) are RBP_ERR_BAD_ARGUMENT before a device is looked for. */
#define RBP_SWEPT_MAX_DEPTH 8
#define RBP_SWEPT_MAX_CELLS 4096             /* the most cells of one piece's box that are scanned */
#define RBP_SWEPT_LIST_BYTES (64u << 20)     /* the work list's budget: 16 Mi items of a chunk of missions */
typedef struct rbp_swept_clearance {
    double  lower_clearance, upper_clearance;   /* 1e9: none */
    double  lower_dist, upper_dist;             /* the readings d_lo and d_up at the two minima (-1: outside or over budget) */
    double  end_time;                           /* Ts[M]: the mission's last segment time, scaled */
    int64_t uncertified, hitting, outside, over_budget, refined;   /* items (agent, segment) */
    int32_t lower_segment, lower_piece, lower_agent, lower_depth;   /* -1: none */
    int32_t upper_segment, upper_piece, upper_agent, upper_depth;
    int32_t status, reserved;                   /* the mission's status; != 0: nothing computed, zeros, indices -1 */
} rbp_swept_clearance;
int rbp_session_swept_clearance(rbp_session* s, int32_t depth, double refine_below, rbp_swept_clearance* out /* [K] */,
                                double* agent_lower /* [K][N] or NULL; host or device pointer */, void* stream);
int rbp_dev_swept_clearance(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T,
                            const double* time_scale, const double* coef, const double* radius,
                            const rbp_world* worlds /* [K]; dist host or device */, int32_t depth, double refine_below,
                            rbp_swept_clearance* out, double* agent_lower);

/* ---- certified intervals for the largest velocity and acceleration of resident plans in CONTINUOUS time ----
 * rbp_dynamics looks at the samples t = j * dt; a peak between two samples is not seen, and timeScale pushes every plan up against its
 * limits (the literal rule RBP_TIMESCALE_FIRST_EIGENVALUES can leave a segment above max_vel).  For an agent a and a segment m (an ITEM)
 * the velocity of an axis is a polynomial of degree 4 and the acceleration one of degree 3; on a PIECE of the segment (piece p of depth D
 * covers [p / 2^D, (p+1) / 2^D] of it) the polynomial lies in the hull of its Bernstein control points and passes through the first and
 * the last one.  So, per axis and derivative, (max_i |b_i| + err) / limit is an upper bound of |X_k(t)| / limit on the piece and
 * max(0, max(|b_0|, |b_n|) - err) / limit a value the curve reaches, err = (16 + 4 D) 2^-53 V a counted rounding term.  All of it -- the
 * derivative's coefficients (the products rbp_dynamics forms), the Bernstein form, the halving, err with its derivation, the order of the
 * peaks -- is the rule of csrc/common/limits_rules.h, which the kernels (kernels/limits.hip) and rbp_limits_host of rbp_host.h share: both
 * return the same bits.  The promise, for the polynomials the double coefficients define and positive limits:
 *     lower_X_ratio <= sup over agents, axes and instants of |X_k(t)| / max_X[a][k] <= upper_X_ratio,   X = vel, acc.
 * upper <= 1 certifies the limit; lower > 1 proves a violation.  uncertified: the items with a piece whose upper ratio, vel or acc, is not
 * <= 1 (a NaN and an infinity count: uncertified == 0 certifies the mission); violating: those with a piece whose lower ratio is > 1.
 * Refinement is fixed: every item is evaluated at depth 0; an item with a depth-0 upper ratio that is not <= refine_above (a NaN goes
 * too) is evaluated again on all 2^depth pieces of depth `depth`, which replace its depth-0 bounds.  depth in 0 .. RBP_LIMITS_MAX_DEPTH;
 * refine_above any number (negative: everything is refined; 1e9: only what is no number below it).  The peaks name the largest ratio
 * and among equal ratios the lexicographically first (segment, piece, agent, axis); a ratio of 0, a negative one or a NaN is never a
 * peak (ratio 0, indices -1: none).  A limit that is not a positive number bounds nothing: its items are uncertified.
 * agent_upper [K][N][2] (NULL: not wanted): an agent's largest upper velocity ratio and largest upper acceleration ratio over its
 * segments and axes, 0 where none, +infinity where one is no number; the row of a mission with a status is left untouched.  It may be
 * a host pointer or a device pointer on the plans' device (classified as rbp_world.dist is; another device: RBP_ERR_BAD_ARGUMENT): a
 * device destination is written in place by the kernels, a host destination goes through one staging buffer and one copy.
 * Memory: items that are refined go through a work list of one uint32 per item, sized for the worst case (every item), of at most
 * RBP_LIMITS_LIST_BYTES; missions are processed in chunks where all of them would need more (a single mission always is one chunk, and
 * one of more than 2^32 - 64 items is refused).  No allocation depends on the data.
 * rbp_session_limits: of a session's K missions, from its own coef, T, time scale, max_vel, max_acc and status, all of which stay in
 *   HBM; waits for an asynchronous solve like every call, enqueues its kernels on `stream`, copies K structs back in one copy and returns
 *   when they have arrived.  Nothing of the session changes.  A mission whose status is not 0 gets that status and nothing computed.
 *   RBP_ERR_BAD_ARGUMENT: a session whose last run did not include the PLANNER stage; and, before a device is looked for, a null
 *   pointer, a depth outside 0 .. RBP_LIMITS_MAX_DEPTH, a refine_above that is no number.  The session's limits are not refused.
 * rbp_dev_limits: the same kernels on a caller's host arrays in rbp_dev_dynamics' layout, uploaded once.  Argument errors (those above,
 *   K, N <= 0, an M[k] outside 1..M_stride, a time scale <= 0, a limit that is not a positive number) are RBP_ERR_BAD_ARGUMENT before a
 *   device is looked for. */
#define RBP_LIMITS_MAX_DEPTH 8
#define RBP_LIMITS_LIST_BYTES (64u << 20)    /* the work list's budget: 16 Mi items of a chunk of missions */
typedef struct rbp_limits {
    double  lower_vel_ratio, upper_vel_ratio;   /* 0: none */
    double  lower_acc_ratio, upper_acc_ratio;
    double  end_time;                           /* Ts[M]: the mission's last segment time, scaled */
    int64_t uncertified, violating, refined;    /* items (agent, segment) */
    int32_t lower_vel_segment, lower_vel_piece, lower_vel_agent, lower_vel_axis, lower_vel_depth;   /* -1: none */
    int32_t upper_vel_segment, upper_vel_piece, upper_vel_agent, upper_vel_axis, upper_vel_depth;
    int32_t lower_acc_segment, lower_acc_piece, lower_acc_agent, lower_acc_axis, lower_acc_depth;
    int32_t upper_acc_segment, upper_acc_piece, upper_acc_agent, upper_acc_axis, upper_acc_depth;
    int32_t status, reserved;                   /* the mission's status; != 0: nothing computed, zeros, indices -1 */
} rbp_limits;
int rbp_session_limits(rbp_session* s, int32_t depth, double refine_above, rbp_limits* out /* [K] */,
                       double* agent_upper /* [K][N][2] or NULL; host or device pointer */, void* stream);
int rbp_dev_limits(int device, int32_t K, int32_t N, const int32_t* M, int32_t M_stride, const double* T,
                   const double* time_scale, const double* coef, const double* max_vel /* [K][N][3] */,
                   const double* max_acc /* [K][N][3] */, int32_t depth, double refine_above, rbp_limits* out,
                   double* agent_upper);

const char* rbp_last_error(void);
int rbp_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* RBP_H */
