/*
 * irlosc.h — C ABI of the MI355X-native batched operational-space controller (libirlosc.so).
 *
 * This is the drop-in boundary that sits UNDER irl_control's Python `OSC.generate()`:
 * the reference has no FFI of its own (it is pure Python/NumPy), so each entry point below names
 * the reference lines whose work it takes over.  Plain pointers and sizes only; no torch types.
 *
 *   reference work                                              -> entry point
 *   ----------------------------------------------------------------------------------------------
 *   OSC.__init__ gain tables (osc.py:19-39), device row masks /
 *   joint sets (device.py:36,66-69; robot.py:28-32,50-55)       -> irlosc_create, irlosc_set_gains
 *   Robot.get_all_states(): M, dq, J stack, EE pose, wrench
 *   (robot.py:44-72,125-136; device.py:115-170; osc.py:132-138) -> irlosc_upload (records assembled by the caller)
 *                                                                  irlosc_upload_raw (assembled on the GPU from raw
 *                                                                  simulator arrays)
 *   targets dict (utils.py:5-67; osc.py:156-159,172)            -> irlosc_set_targets
 *   OSC.generate numerical body (osc.py:41-118,144-200)         -> irlosc_step / irlosc_step_device
 *   forces gather u_all[actuator_trnids] (osc.py:203-210)       -> host side, from u[B,n]
 *   the per-tick MuJoCo reads themselves: mj_fullM (robot.py:68-72),
 *   jacp / jacr (device.py:115-133), qfrc_bias (osc.py:190-191),
 *   EE xpos / xquat (device.py:97-99), from (qpos, qvel)        -> irlosc_set_model, irlosc_upload_q, then irlosc_frontend
 *                                                                  (dense records) or irlosc_step_from_q (fused: no records);
 *                                                                  irlosc_step_from_q_device from the caller's HBM
 *   the per-tick F/T reads rotated by the ft_frame_* site frames
 *   (device.py:135-170) on the path from joint coordinates      -> irlosc_set_ft_sensors, irlosc_set_sensordata
 *
 * Record layouts (batch-major, row-major, element type = cfg.dtype: float or double):
 *   M[B][n][n]      joint-space inertia, symmetric positive definite (the row16 kernels read row j as column j)
 *   J[B][k][n]      stacked task Jacobian, device blocks in TARGETS order, k = sum(dev_rows)
 *   dq[B][n]        joint velocities
 *   bias[B][n]      qfrc_bias (gravity + Coriolis); ignored unless IRLOSC_USE_G
 *   ee_pose[B][ndev][7]   x y z qw qx qy qz of each target device's end effector
 *   tgt_pose[B][ndev][7]  target x y z qw qx qy qz (quaternion need not be normalised)
 *   tgt_vel[B][ndev][6]   hstack(xyz_vel, abg_vel) or NULL (= all zero -> damping branch A)
 *   wrench[B][ndev][6]    world-frame F/T sensor reading or NULL; used only with IRLOSC_ADMITTANCE
 *   u[B][n]         joint torques u_all (osc.py:152-200)
 *   flags[B]        uint32 status bits per instance (IRLOSC_FLAG_*)
 *
 * Contracts the kernels rely on (not checked on the device):
 *   - M is symmetric: the throughput kernels read row j of M as its column j (the generic kernel uses M as given, like
 *     osc.py:49,151).  Records that come from the HOST are probed on the device: irlosc_upload and irlosc_tick return
 *     IRLOSC_ERR_ARG when an instance has max |M - M^T| > 1e-6 max |M| (over its FINITE entries: a robot whose M holds
 *     NaN / Inf is not refused -- it is reported per instance through IRLOSC_FLAG_NONFINITE / M_NOT_PD and the other robots
 *     of the batch get their torques) and the context runs a throughput kernel.  Records
 *     assembled on the device (irlosc_upload_raw / irlosc_assemble_device / irlosc_frontend) are symmetric by
 *     construction; for irlosc_step_device it stays the caller's contract;
 *   - (not a contract, an observation the library makes for itself) records of a real robot carry the zeros of its kinematic
 *     tree -- robot.py:68-72 / device.py:115-133 hand over what mj_fullM / mj_jacBody wrote -- and uploads are probed for
 *     them: see irlosc_slot_structure;
 *   - device pointers handed to irlosc_step_device / irlosc_assemble_device are 16-byte aligned;
 *   - a context is driven from ONE stream at a time: its train tables, worklists and pending stage-2 work are ordered
 *     by stream order only, so a caller stream passed to the *_device entry points must not run concurrently with the
 *     context's own stream or with another caller stream on the same context;
 *   - a step over B instances needs B instances of state and of targets in the slot (IRLOSC_ERR_STATE otherwise).
 *
 * Ownership: the caller owns every host buffer (borrowed for the duration of the call); the
 * library owns its device buffers and its HIP stream.  Errors: 0 = success, negative irlosc_status
 * otherwise, message via irlosc_last_error(); nothing throws across the ABI.  A context is bound
 * to one GPU and is not thread-safe; distinct contexts may be driven from distinct threads.
 * There is NO CPU fallback: every compute entry point fails with IRLOSC_ERR_HIP without a GPU.
 */
#ifndef IRLOSC_H
#define IRLOSC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): a fused irlosc_step_from_q invalidates the slot's dense records (IRLOSC_ERR_STATE on a later irlosc_step);
 * IRLOSC_KERNEL_AUTO on float32 records means fp64 arithmetic (row16 "mixed": there is no fp32-arithmetic kernel); every n = 25 layout
 * (k <= 16, ndev <= 4) has a row16-class kernel; irlosc_kernel_class / irlosc_giveup_counts / irlosc_time_trains added;
 * only the irlosc_* symbols are exported.  _lib.py refuses a library whose version differs. */
#define IRLOSC_ABI_VERSION 3
/* the entry points below are the ONLY dynamic symbols of libirlosc.so (built with -fvisibility=hidden) */
#define IRLOSC_API __attribute__((visibility("default")))
#define IRLOSC_MAX_DEV 4
#define IRLOSC_MAX_N 32
#define IRLOSC_MAX_K 16
#define IRLOSC_GAIN_WORDS 12 /* kp kv ko k0 k1 k2 d0 d1 d2 max_vel0 max_vel1 has_max_vel */

typedef enum { IRLOSC_F32 = 0, IRLOSC_F64 = 1 } irlosc_dtype;

typedef enum {
    IRLOSC_OK = 0,
    IRLOSC_ERR_ARG = -1,     /* bad argument / layout */
    IRLOSC_ERR_HIP = -2,     /* HIP runtime error (no device, OOM, launch failure) */
    IRLOSC_ERR_STATE = -3    /* call order (e.g. step before upload) */
} irlosc_status;

/* cfg.flags */
#define IRLOSC_USE_G      1u  /* add bias forces, osc.py:190-191 */
#define IRLOSC_ADMITTANCE 2u  /* add ext_f to the task signal, osc.py:184-185 */
#define IRLOSC_NULLSPACE  4u  /* null-space damping, osc.py:195-200 */

/* per-instance status bits written by the kernels */
#define IRLOSC_FLAG_M_NOT_PD      1u   /* Cholesky of M met a non-positive pivot */
#define IRLOSC_FLAG_PINV_BRANCH   2u   /* |det(J M^-1 J^T)| < 1e-4: reference takes np.linalg.pinv (osc.py:55) */
#define IRLOSC_FLAG_EIGEN_PATH    4u   /* k x k eigen-decomposition was needed (not certifiably cond < 1e5) */
#define IRLOSC_FLAG_TRUNCATED     8u   /* at least one eigenvalue <= 1e-5 * max was dropped */
#define IRLOSC_FLAG_VEL_BRANCH_B 16u   /* some device had all six target-velocity components non-zero (osc.py:173-177) */
#define IRLOSC_FLAG_BAD_JIDX     32u   /* branch B indexed dx out of range (IndexError in the reference) */
#define IRLOSC_FLAG_NONFINITE    64u   /* output contains NaN/Inf */

/* kernel selection (cfg.kernel) */
#define IRLOSC_KERNEL_AUTO    0   /* fp64 ARITHMETIC always (the reference's, osc.py:49-55; meets 1e-5): row16 for every n = 25
                                     layout -- on float64 records and on float32 records alike -- else generic */
#define IRLOSC_KERNEL_GENERIC 1   /* one wavefront per instance, LDS tiles, any n<=32, k<=16 */
#define IRLOSC_KERNEL_REMOVED_GROUP 2 /* (ABI versions 1-2: an fp32-ARITHMETIC kernel, error ~ eps32 * cond(J M^-1 J^T) -- 14 % of physical
                                     instances missed the 1e-5 contract.  Removed in version 3: irlosc_create answers IRLOSC_ERR_ARG.) */
#define IRLOSC_KERNEL_ROW16   3   /* fp64 arithmetic: 16 lanes (one DPP row) per instance, broadcast-FMA formulation (n = 25;
                                     instantiations for (k, ndev) = (13,3), (12,2), (7,3), (6,2), KMAX-padded variants for every
                                     other k <= 16, ndev <= 4: irlosc_kernel_class); float32 records = the "mixed" path */

typedef struct irlosc_cfg {
    int32_t hip_device;                      /* HIP device ordinal */
    int32_t dtype;                           /* irlosc_dtype */
    int32_t max_batch;                       /* capacity B_max of the resident buffers */
    int32_t n_slots;                         /* >=1 resident input sets (bench rotates them to defeat the 256 MiB L3) */
    int32_t n;                               /* robot.num_joints_total (robot.py:32) */
    int32_t ndev;                            /* number of target devices, targets order */
    uint32_t flags;                          /* IRLOSC_USE_G | IRLOSC_ADMITTANCE | IRLOSC_NULLSPACE */
    int32_t kernel;                          /* IRLOSC_KERNEL_* */
    int32_t dev_rows[IRLOSC_MAX_DEV];        /* r_d = popcount(ctrlr_dof[d]) */
    uint8_t ctrlr_dof[IRLOSC_MAX_DEV][6];    /* row mask hstack(ctrlr_dof_xyz, ctrlr_dof_abg), device.py:36 */
    uint8_t calc_xyz[IRLOSC_MAX_DEV];        /* np.sum(device.ctrlr_dof_xyz) > 0, osc.py:108 */
    uint8_t calc_abg[IRLOSC_MAX_DEV];        /* np.sum(device.ctrlr_dof_abg) > 0, osc.py:113 */
    uint32_t joint_mask[IRLOSC_MAX_DEV];     /* bit j set <=> j in device.joint_ids_all (osc.py:174) */
    int32_t j_idx0[IRLOSC_MAX_DEV];          /* first row of J_idxs[name] (robot.py:50-55), used by branch B */
} irlosc_cfg;

typedef struct irlosc_ctx irlosc_ctx;

IRLOSC_API int irlosc_abi_version(void);

/* Number of HIP devices visible, or a negative irlosc_status. */
IRLOSC_API int irlosc_device_count(void);

IRLOSC_API int irlosc_create(const irlosc_cfg* cfg, irlosc_ctx** out);
IRLOSC_API void irlosc_destroy(irlosc_ctx* ctx);
IRLOSC_API const char* irlosc_last_error(const irlosc_ctx* ctx); /* ctx may be NULL: last create() error */
IRLOSC_API const char* irlosc_kernel_name(const irlosc_ctx* ctx); /* name of the kernel irlosc_step launches */
/* What irlosc_create settled on, for a C caller that asked for IRLOSC_KERNEL_AUTO and wants to know whether it got a throughput
 * kernel: IRLOSC_CLASS_GENERIC means the one-wavefront-per-instance kernel (any n <= 32: ~25x slower per instance at large batches;
 * AUTO only lands there when n != 25).  ROW16 = an instantiation for exactly this (k, ndev); ROW16_PADDED = the row16 kernel of the
 * smallest tier KMAX in {4, 7, 10, 13, 16} >= k, with k and ndev as run-time arguments (same results bit for bit, a few per cent to
 * a third slower than an exact instantiation would be; the name then ends in "_ndev<d>_pad<KMAX>").
 * One difference in HOW a result is reached, not in the result: a task row no joint can move (an exact zero row of J) is taken out of
 * the k x k factorisation up front by the padded kernels and by the lane-per-robot step of the fused path (PINV and TRUNCATED set, no
 * eigen stage needed for it), while the four exact instantiations find it in their eigen stage (three such directions at most, then the
 * give-up list -> generic kernel).  Torques agree to rounding and the flags PINV / TRUNCATED agree; irlosc_giveup_counts and the
 * throughput on such inputs differ.  No layout of the shipped examples has such a row. */
#define IRLOSC_CLASS_GENERIC      0
#define IRLOSC_CLASS_ROW16        1
#define IRLOSC_CLASS_ROW16_PADDED 2
IRLOSC_API int irlosc_kernel_class(const irlosc_ctx* ctx);
IRLOSC_API const char* irlosc_frontend_name(const irlosc_ctx* ctx); /* name of the kernel irlosc_frontend launches ("" before irlosc_set_model) */

/* gains[nb][ndev][IRLOSC_GAIN_WORDS] and null_kv[nb] as double; nb == 1 broadcasts one gain set to
 * every instance (kept in constant/SGPR space), nb == max_batch gives per-instance gains. */
IRLOSC_API int irlosc_set_gains(irlosc_ctx* ctx, const double* gains, const double* null_kv, int32_t nb);

/* Host -> device copy of one batch of robot state into resident slot `slot`.  wrench may be NULL.  On the throughput paths
 * an asymmetric M is refused (IRLOSC_ERR_ARG, the slot then holds nothing): see the contracts block above. */
IRLOSC_API int irlosc_upload(irlosc_ctx* ctx, int32_t slot, int32_t B, const void* M, const void* J,
                  const void* dq, const void* bias, const void* ee_pose, const void* wrench);
/* 1 when the records now in `slot` carry the zero pattern of the compiled Dual-UR5 tree and the fp64 row16 kernel will
 * therefore run its factorisation in the tree-structured form (M = L^T L from the leaves up, fill-in free: Featherstone's
 * branch-induced sparsity; rows of Y = L^-T J^T under no end effector skipped), 0 when it runs the dense recursion.  The
 * verdict is taken when the records arrive: irlosc_upload / irlosc_upload_raw look at every instance (one pass on the device:
 * M[i][j] exactly 0 unless hinge i is above hinge j or j above i; columns of J exactly 0 for hinges that move no end-effector
 * candidate -- what mj_fullM / mj_jacBody leave, robot.py:68-72, device.py:115-133), batches of 64 instances and more only;
 * irlosc_frontend's lane kernel writes such records by construction; irlosc_assemble_device (caller's stream) does not
 * qualify until irlosc_probe_structure has looked.  The form is chosen per slot: a train of irlosc_step_resident that mixes
 * qualifying and other slots is issued as two launches.  Results differ from the dense recursion at rounding level only.  IRLOSC_TREE=0 in the environment turns the
 * form off. */
IRLOSC_API int irlosc_slot_structure(const irlosc_ctx* ctx, int32_t slot);
/* The same look at records that are already in `slot` (first B instances), for the one path that cannot take it by itself:
 * irlosc_assemble_device on a caller's stream.  Synchronous on the context's stream -- the caller synchronises its own stream
 * first.  Returns 1 / 0 like irlosc_slot_structure (and updates that verdict), or a negative irlosc_status. */
IRLOSC_API int irlosc_probe_structure(irlosc_ctx* ctx, int32_t slot, int32_t B);
/* Which kernels a step of B instances on `slot` runs (B <= 0: the instances the slot holds).  IRLOSC_ROUTE_LANE: the resident lane
 * route -- float64 records of an IRLOSC_KERNEL_AUTO context in the tree-structured form, a model set whose layout has a lane tier
 * (irlosc_from_q_name names it), no target velocities, B >= 4096.  Records that qualify are packed once, when they enter the slot
 * (irlosc_upload / irlosc_upload_raw / irlosc_upload_raw_sparse / irlosc_frontend / irlosc_probe_structure), into a compact block of
 * the tree's non-zeros (3.1 KB per robot, allocated by the slot's first pack); irlosc_step and irlosc_step_resident then run the
 * lane-per-robot OSC step of the fused path on that block, the robots it gives up on the generic kernel on the dense records, which
 * stay in the slot.  Results differ from the row16 kernel at rounding level; flags are the same.  IRLOSC_RESIDENT_LANE=0 in the
 * environment (read at irlosc_create) turns the route off.  kernel_name / kernel_class do not change with the route. */
#define IRLOSC_ROUTE_NONE       0      /* bad handle or slot */
#define IRLOSC_ROUTE_GENERIC    1
#define IRLOSC_ROUTE_ROW16      2      /* row16 kernel, dense recursion */
#define IRLOSC_ROUTE_ROW16_TREE 3      /* row16 kernel, tree-structured form */
#define IRLOSC_ROUTE_LANE       4      /* lane-per-robot OSC step on the slot's compact block */
IRLOSC_API int irlosc_slot_route(const irlosc_ctx* ctx, int32_t slot, int32_t B);
/* Host -> device copy of the targets for slot `slot`.  tgt_vel may be NULL (all zero). */
IRLOSC_API int irlosc_set_targets(irlosc_ctx* ctx, int32_t slot, int32_t B, const void* tgt_pose,
                       const void* tgt_vel);

/* One control step over the B instances of `slot`: launch, then copy u[B][n] (and flags[B], may
 * be NULL) back to the host buffers.  u_host may be NULL to leave the result on the device. */
IRLOSC_API int irlosc_step(irlosc_ctx* ctx, int32_t slot, int32_t B, void* u_host, uint32_t* flags_host);

/* Benchmark form: `iters` back-to-back steps on resident data, slot = (first_slot + i) % n_slots,
 * no host copies.  Consecutive steps are independent batches, so the throughput path chains several of them
 * into one launch and lets the eigen-path stage of a launch's steps ride in the next launch; everything is
 * complete when the call returns, and irlosc_download then yields the LAST step's outputs.  *ms_total receives
 * the HIP-event time of the whole region on the library's own stream; *ms_kernel_avg = *ms_total / iters. */
IRLOSC_API int irlosc_step_resident(irlosc_ctx* ctx, int32_t first_slot, int32_t B, int32_t iters,
                         float* ms_total, float* ms_kernel_avg);

/* Roofline support: mean duration of the DOMINANT kernel launch, measured live with one HIP event pair per launch
 * on the library's stream, over about `iters` (<= 256) steps run exactly like irlosc_step_resident.  Group path:
 * the fused launch (stage 1 of irlosc_steps_per_launch() chained steps + the riding stage 2 of the previous
 * launch's steps); generic path: the generic kernel.  Outputs are complete, as after irlosc_step_resident. */
IRLOSC_API int irlosc_time_dominant_kernel(irlosc_ctx* ctx, int32_t slot, int32_t B, int32_t iters, float* ms_avg);
/* Roofline evidence WITHOUT a tracer ("Timing method"; row16 kernel only).  `ntrains` (<= 4096) consecutive
 * trains of irlosc_steps_per_launch() steps, issued exactly as irlosc_step_resident issues them (slots rotating from first_slot),
 * after one untimed train.  Every train gets (a) its own HIP event pair on the library's stream and (b) the wall clock
 * (s_memrealtime, 100 MHz) stamped by its main kernel itself: the start of its first wave and the end of its last wave.
 *   out[4 i + 0]  event pair of train i in milliseconds (main kernel + give-up pass; from_q: walk + OSC kernel + give-up pass)
 *   out[4 i + 1]  start of train i's first wave, microseconds after the first wave of train 0
 *   out[4 i + 2]  end of train i's last wave, same origin
 *   out[4 i + 3]  shader clock in MHz during train i: cycle counter against wall clock over the life of one sample wave (the kernel is
 *                 fp64-VALU-heavy and the part power-limited: 1.5-1.8 GHz under this load against the 2.4 GHz peak, and box to box different)
 * => in-kernel duration of train i = out[4 i + 2] - out[4 i + 1] (what a kernel trace reports per dispatch, minus the
 * tracer's own serialisation); steady-state period = out[4 (i + 1) + 1] - out[4 i + 1] (what irlosc_step_resident's wall
 * time divided by the number of trains measures).  from_q != 0: trains of irlosc_step_resident_from_q (the stamps are the OSC
 * kernel's; the walk in front of it is inside the period and the event pair). */
IRLOSC_API int irlosc_time_trains(irlosc_ctx* ctx, int32_t first_slot, int32_t B, int32_t ntrains, int32_t from_q, double* out);
/* How many instances the most recent step (out[0]) / the steps of the most recent train (out[0 .. irlosc_steps_per_launch() - 1]) handed
 * from the row16 kernel's in-wave eigen stage to the generic kernel -- task spaces that lose MORE than three directions at once
 * (osc.py:55 with four or more singular values under the cut).  Results are the same either way; throughput is not: the give-up
 * pass is a serial tail of its train (one instance costs ~27 us per train, a batch dominated by them runs at 4.5e6 steps/s instead of
 * 6e8).  Zero on physical states of the Dual-UR5 in every sweep so far; a caller whose task sets are rank-deficient by construction
 * can watch this counter.  out[8]; all zero on the other kernels.  (A train that mixes tree-form and dense slots is two launches;
 * every step still reports at its own index of the train.)  Synchronises the context's stream. */
IRLOSC_API int irlosc_giveup_counts(irlosc_ctx* ctx, int32_t* out);
/* Steps chained in one launch by irlosc_step_resident / irlosc_time_dominant_kernel (1 on the generic path):
 * the algorithmic bytes of one dominant launch = this many steps' worth. */
IRLOSC_API int irlosc_steps_per_launch(const irlosc_ctx* ctx);

/* State assembly on the GPU (what Robot.get_all_states() / Device.get_state() do per robot on the host:
 * robot.py:44-72,125-136; device.py:115-170): one batch of RAW simulator arrays in, the resident records of slot
 * `slot` out (M, J, dq, bias, ee_pose, wrench), same result as irlosc_upload of host-assembled records.
 *   qM[B][nv][nv]            dense inertia matrix (mj_fullM), nv = sim.model.nv (may exceed n: free bodies)
 *   qvel[B][nv], qfrc_bias[B][nv]
 *   jacp[B][ndev][3][nv], jacr[B][ndev][3][nv]   EE-body Jacobians of the target devices, targets order
 *   ee_xpos[B][ndev][3], ee_xquat[B][ndev][4]    EE-body pose (w,x,y,z)
 *   site_xmat[B][ndev][9], sensordata[B][n_sensor]   F/T site frames and raw sensor readings; both may be NULL
 *                                                    (wrench = 0), devices without a sensor have ft_force0 = -1
 * The row mask ctrlr_dof and the block order come from the context's cfg. */
typedef struct irlosc_raw_desc {
    int32_t nv;                               /* dofs in the scene (columns of the raw Jacobians) */
    int32_t n_sensor;                         /* sensordata length per instance */
    int32_t joint_ids[IRLOSC_MAX_N];          /* robot.joint_ids_all: raw dof of robot position p (robot.py:28-32) */
    int32_t dq_src[IRLOSC_MAX_N];             /* raw dof whose qvel lands in dq[p], -1 = 0 (robot.py:60-65) */
    int32_t ft_force0[IRLOSC_MAX_DEV];        /* first sensordata index of the force triple, -1 = no sensor (device.py:139-170) */
    int32_t ft_torque0[IRLOSC_MAX_DEV];
} irlosc_raw_desc;
IRLOSC_API int irlosc_upload_raw(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_raw_desc* desc, const void* qM,
                      const void* qvel, const void* qfrc_bias, const void* jacp, const void* jacr,
                      const void* ee_xpos, const void* ee_xquat, const void* site_xmat, const void* sensordata);

/* The same with M as MuJoCo itself holds it: mjData.qM, the sparse lower triangle over the kinematic tree -- nM values per instance,
 * dof i's run starts at dof_Madr[i] and walks UP the tree: M[i][i], M[i][parent(i)], M[i][parent(parent(i))], ... with parent =
 * mjModel.dof_parentid (-1 ends the run).  The expansion mj_fullM does on the host (robot.py:68-72 calls it for every robot and tick)
 * runs on the GPU instead, inside the assembly kernel: 1.4 KB instead of 5 KB (nv = 25) or 11 KB (nv = 37) per robot cross PCIe.
 * qM_sparse[B][nM] in the context's dtype; everything else as irlosc_upload_raw. */
#define IRLOSC_MAX_NV 128
typedef struct irlosc_qm_layout {
    int32_t nM;                               /* mjModel.nM */
    int32_t dof_Madr[IRLOSC_MAX_NV];          /* mjModel.dof_Madr[0 .. nv) */
    int32_t dof_parentid[IRLOSC_MAX_NV];      /* mjModel.dof_parentid[0 .. nv) */
} irlosc_qm_layout;
IRLOSC_API int irlosc_upload_raw_sparse(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_raw_desc* desc, const irlosc_qm_layout* qml,
                             const void* qM_sparse, const void* qvel, const void* qfrc_bias, const void* jacp, const void* jacr,
                             const void* ee_xpos, const void* ee_xquat, const void* site_xmat, const void* sensordata);

/* Same assembly for simulators whose state already lives in HBM: every array pointer is a DEVICE pointer (layouts
 * as above), hip_stream a hipStream_t (NULL = the context's stream).  No copies; the call returns after enqueueing the
 * kernel, and steps of this context issued on the same stream see the assembled slot. */
IRLOSC_API int irlosc_assemble_device(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_raw_desc* desc, const void* d_qM,
                           const void* d_qvel, const void* d_qfrc_bias, const void* d_jacp, const void* d_jacr,
                           const void* d_ee_xpos, const void* d_ee_xquat, const void* d_site_xmat,
                           const void* d_sensordata, void* hip_stream);

IRLOSC_API int irlosc_download(irlosc_ctx* ctx, int32_t B, void* u_host, uint32_t* flags_host);
IRLOSC_API int irlosc_sync(irlosc_ctx* ctx);          /* waits for the context's stream */
IRLOSC_API int irlosc_device_sync(irlosc_ctx* ctx);   /* hipDeviceSynchronize on the context's GPU (bench bracket) */

/* One control tick in ONE call (what OSC.generate does per tick for B robots, osc.py:120-210): the records are packed
 * into a pinned staging block, cross PCIe in one copy, the step runs on them in place, u[B][n] and flags[B] come back
 * in one copy, and the call synchronises once.  Same record layouts as irlosc_upload / irlosc_set_targets; wrench and
 * tgt_vel may be NULL.  Does not touch the resident slots. */
IRLOSC_API int irlosc_tick(irlosc_ctx* ctx, int32_t B, const void* M, const void* J, const void* dq, const void* bias,
                const void* ee_pose, const void* wrench, const void* tgt_pose, const void* tgt_vel, void* u_host,
                uint32_t* flags_host);

/* Raw-device-pointer form for callers that already hold the state in HBM (e.g. an on-GPU
 * simulator): same layouts as above, all pointers are device pointers, hip_stream is a
 * hipStream_t (NULL = the context's stream).  No copies, no synchronisation. */
IRLOSC_API int irlosc_step_device(irlosc_ctx* ctx, int32_t B, const void* dM, const void* dJ, const void* ddq,
                       const void* dbias, const void* dee_pose, const void* dtgt_pose,
                       const void* dtgt_vel, const void* dwrench, void* du, uint32_t* dflags,
                       void* hip_stream);

/* ---- rigid-body front end: joint coordinates in, records assembled on the GPU -----------
 * Replaces the per-tick reads the reference makes from MuJoCo on the host - mj_fullM (robot.py:68-72), the EE-body
 * Jacobians jacp / jacr (device.py:115-133), qfrc_bias (osc.py:190-191), EE xpos / xquat (device.py:97-99) - by forward
 * kinematics, Jacobians, composite-rigid-body M and recursive-Newton-Euler bias forces computed from (qpos, qvel) for the
 * whole batch.  The model is a tree of bodies, each welded to its parent or attached by ONE hinge (MuJoCo conventions:
 * body frame pos + quat relative to the parent, hinge axis / anchor in the body frame, inertial frame ipos + iquat with
 * principal moments, quaternions w x y z).  Bodies must be listed parents first (MuJoCo's numbering does that);
 * joint j of the model is position j of the n-vector (n = cfg.n).  ee_body[d] = body whose frame is target device d's
 * end effector (targets order).  The F/T wrench is not a function of (qpos, qvel): without a sensor feed it stays whatever
 * irlosc_upload / irlosc_upload_raw last put into the slot (absent: zero); with one (irlosc_set_ft_sensors + irlosc_set_sensordata,
 * below) every step from joint coordinates rotates the slot's sensor readings by the F/T site frames of its own forward kinematics. */
#define IRLOSC_MAX_BODIES 64
typedef struct irlosc_model {
    int32_t nb;                               /* bodies, <= IRLOSC_MAX_BODIES */
    int32_t nj;                               /* hinges, must equal cfg.n */
    int32_t parent[IRLOSC_MAX_BODIES];        /* -1 = world */
    int32_t joint_of_body[IRLOSC_MAX_BODIES]; /* hinge index, or -1 = welded to the parent */
    double pos[IRLOSC_MAX_BODIES][3];
    double quat[IRLOSC_MAX_BODIES][4];
    double jaxis[IRLOSC_MAX_N][3];            /* unit axis, body frame */
    double jpos[IRLOSC_MAX_N][3];             /* anchor, body frame */
    double armature[IRLOSC_MAX_N];
    double mass[IRLOSC_MAX_BODIES];
    double ipos[IRLOSC_MAX_BODIES][3];
    double iquat[IRLOSC_MAX_BODIES][4];
    double inertia[IRLOSC_MAX_BODIES][3];     /* principal moments in the inertial frame */
    double gravity[3];
    int32_t ee_body[IRLOSC_MAX_DEV];
} irlosc_model;
/* Validates the tree (parents precede children, one body per hinge, masses >= 0) and allocates per slot qpos / qvel of
 * max_batch robots.  A model with the compiled Dual-UR5 tree shape selects the lane-per-robot kernel -- its side buffer of
 * ceil(max_batch / 64) x 266 x 512 bytes (139 MB at 65 536 robots) is allocated by the first irlosc_frontend; if that fails the
 * context drops to the generic kernel -- any other tree the generic kernel.  The fused path's walk (irlosc_step_from_q) exists twice
 * for that shape: with the structural constants of the Dual-UR5's MJCF compiled in (body frames not rotated against / coincident with
 * their parent's, hinges about coordinate axes through their body's origin, inertial frames aligned with the body frame: csrc/topo_dual_ur5.hpp,
 * TopoDualUr5S) and shape-only; the model's numbers are checked against those constants here and decide which one runs
 * (irlosc_from_q_name says: "..._dual_ur5_s + ..." is the first). */
IRLOSC_API int irlosc_set_model(irlosc_ctx* ctx, const irlosc_model* model);
/* Joint positions and velocities of one batch into resident slot `slot`: qpos[B][n], qvel[B][n], always double.  On a context whose
 * model takes the fused path the library keeps a second copy in the walk's own layout ([ceil(B / 64)][2 n][64 robots]: a hinge's pair is two
 * coalesced loads), written by a small kernel behind the copies. */
IRLOSC_API int irlosc_upload_q(irlosc_ctx* ctx, int32_t slot, int32_t B, const double* qpos, const double* qvel);
/* Run the front end on the slot's (qpos, qvel): fills its M, J, dq, bias, ee_pose records (asynchronous, context's
 * stream); irlosc_set_targets + irlosc_step then work as after irlosc_upload.  Afterwards the slot holds the records of
 * exactly B robots (an earlier, larger upload no longer vouches for the instances beyond B); the wrench of the slot stays what
 * the last irlosc_upload / irlosc_upload_raw wrote (undefined for instances beyond THAT call's B). */
IRLOSC_API int irlosc_frontend(irlosc_ctx* ctx, int32_t slot, int32_t B);
/* Copy records of slot `slot` back to the host (any pointer may be NULL): what irlosc_upload put there, or what the front
 * end / irlosc_upload_raw assembled on the GPU.  Same layouts and element type as irlosc_upload. */
IRLOSC_API int irlosc_download_records(irlosc_ctx* ctx, int32_t slot, int32_t B, void* M, void* J, void* dq, void* bias,
                            void* ee_pose);
/* One control step from joint coordinates: irlosc_upload_q + irlosc_set_targets, then this (results as after irlosc_step).
 * With the compiled Dual-UR5 tree shape and the fp64 row16 kernel this is the FUSED path: the lane-per-robot walk leaves only
 * the structural non-zeros of M and J, the bias forces and the EE poses in a compact exchange buffer (2.6 KB per robot,
 * written once, coalesced) and the OSC kernel gathers its operands from there -- the dense records of the slot are neither
 * written nor read -- except that robots the in-kernel eigen stage hands to the generic kernel get theirs from the
 * wave-per-robot front end, into the slot.  AFTER A FUSED STEP THE SLOT THEREFORE HOLDS NO RECORDS: irlosc_step,
 * irlosc_step_resident and irlosc_download_records on it fail with IRLOSC_ERR_STATE until irlosc_frontend / irlosc_upload* fills
 * it again (its joint coordinates and targets stay).  Other models / kernels: irlosc_frontend + irlosc_step (records left behind).
 * The exchange buffers (ceil(max_batch / 64) x 334 x 512 bytes each: 318 entries of the walk + IRLOSC_MAX_K rows for the gained task error
 * that a task pass between the walk and the OSC kernel leaves; 175 MB at 65 536 robots) are allocated by the first fused step: one for this call,
 * one per step of a train (8) for irlosc_step_resident_from_q; if that allocation fails the context drops to the path through
 * dense records.
 * The OSC step behind the walk (ABI version 3): for a layout whose task rows fit an instantiation -- at most six rows per arm and one on
 * the stand: every layout of the shipped examples -- and a train without target velocities it runs ONE LANE PER ROBOT on the exchange
 * buffer (tree-structured L^T L, Y, A = J M^-1 J^T, the k x k factorisation, certificate, solve and torques, with part 1 of the task signal
 * computed in the same kernel); the robots whose solve is a truncated pseudo-inverse (osc.py:55; ~15 % of physical states) leave a 1.5 KB
 * record and are finished by an eigen pass -- one lane per robot too where a step flags 3 000 robots or more, four records per wave on
 * thinner lists, chosen on the device per step --, what that gives up on goes to the generic kernel as before.  Everything else takes
 * the row16 FROMQ kernel (behind a task pass).  Same contract either way (1e-5 on the parity domain, same flags); irlosc_from_q_name
 * says which.  The lane form's records -- max_batch (rounded up to 64) x 1 536 bytes per step of a train -- are allocated with the
 * exchange buffers; if that fails only the lane form is switched off.  Environment switches for A/B measurements: INTEGRATION.md. */
IRLOSC_API int irlosc_step_from_q(irlosc_ctx* ctx, int32_t slot, int32_t B, void* u_host, uint32_t* flags_host);
/* What irlosc_step_from_q / irlosc_step_resident_from_q launch ("" before irlosc_set_model). */
IRLOSC_API const char* irlosc_from_q_name(const irlosc_ctx* ctx);
/* Benchmark form of the whole path from joint coordinates: `iters` steps like irlosc_step_from_q on resident (qpos, qvel),
 * chained into trains on the fused path, slot = (first_slot + i) % n_slots; HIP-event time of the region on the library's
 * stream. */
IRLOSC_API int irlosc_step_resident_from_q(irlosc_ctx* ctx, int32_t first_slot, int32_t B, int32_t iters, float* ms_total,
                                float* ms_step_avg);

/* ---- F/T sensor feed of the path from joint coordinates (irl_control/device.py:135-170, osc.py:179-185) -----------------
 * The reference reads the F/T sensors every tick and rotates force sensordata[f0 .. f0 + 3] and torque sensordata[t0 .. t0 + 3]
 * of target device d into the world by the frame of the site ft_frame_<device> (site_xmat).  On the path from joint coordinates
 * that frame comes from the step's own forward kinematics: the site's body is welded to the device's end effector, so
 * R(site) = R(ee_quat) R_rel[d] with a constant R_rel[d] = R(ee)^T R(site), and
 *     wrench[b][d] = (R(ee_quat) R_rel[d] force, R(ee_quat) R_rel[d] torque)      (devices without a sensor: zero)
 * is used exactly as a record wrench is (IRLOSC_ADMITTANCE; without it the feed is accepted and changes nothing, as in the
 * reference).  One small kernel per train (osc_ft_wrench, one lane per robot) between the walk and the OSC step -- or, on the path
 * through dense records, between irlosc_frontend's kernel and the step; a context whose slots have no feed launches exactly what
 * it launched before. */
typedef struct irlosc_ft_desc {
    int32_t n_sensor;                         /* sensordata length per robot (doubles) */
    int32_t site_body[IRLOSC_MAX_DEV];        /* body carrying target device d's F/T site (mjModel.site_bodyid); -1 = no sensor */
    double site_quat[IRLOSC_MAX_DEV][4];      /* site frame in that body, w x y z (mjModel.site_quat; need not be normalised) */
    int32_t ft_force0[IRLOSC_MAX_DEV];        /* first sensordata index of the force triple (as irlosc_raw_desc) */
    int32_t ft_torque0[IRLOSC_MAX_DEV];
} irlosc_ft_desc;
/* After irlosc_set_model (IRLOSC_ERR_STATE before).  Checked for every device with a sensor (IRLOSC_ERR_ARG naming the device
 * otherwise): n_sensor >= 3, both indices in [0, n_sensor - 3], site_body a body of the model, and the site body RIGIDLY attached to
 * the device's ee_body -- no hinge on the tree path between the two, in either direction (the shipped model: the site body
 * robotiq_85_adapter_link_* is a welded child of ur_EE_*).  R_rel[d] is computed here, on the host, from the model's body
 * quaternions.  Replaces an earlier description and clears every slot's sensor feed (laid out for that one); a later irlosc_set_model
 * clears the description and every feed too. */
IRLOSC_API int irlosc_set_ft_sensors(irlosc_ctx* ctx, const irlosc_ft_desc* desc);
/* Host -> device copy of sensordata[B][n_sensor] (always double, like qpos) into slot `slot`'s feed: from then on the slot's sensors
 * are the wrench source of every step from joint coordinates on it (irlosc_step_from_q, irlosc_step_resident_from_q; fused and
 * through dense records alike), the record wrench is left alone.  The buffer (max_batch x n_sensor x 8 bytes: 9.4 MB at 65 536 x 18)
 * is allocated by the slot's first feed.  B = 0 or sensordata = NULL clears the feed (the record wrench is the source again), and so
 * does any irlosc_upload* / irlosc_assemble_device of the slot (they bring a wrench of their own).  A step from joint coordinates
 * over more robots than the feed holds fails with IRLOSC_ERR_STATE.  Needs irlosc_set_ft_sensors (IRLOSC_ERR_STATE).  Synchronous,
 * like irlosc_upload_q. */
IRLOSC_API int irlosc_set_sensordata(irlosc_ctx* ctx, int32_t slot, int32_t B, const double* sensordata);
/* One step from joint coordinates on caller-owned DEVICE arrays (what irlosc_step_device is to irlosc_step):
 *   d_qpos, d_qvel[B][n]             double
 *   d_tgt_pose[B][ndev][7]           context dtype; d_tgt_vel[B][ndev][6] or NULL (all zero), as irlosc_set_targets
 *   d_sensordata[B][n_sensor]        double, or NULL (zero wrench); non-NULL needs irlosc_set_ft_sensors (IRLOSC_ERR_STATE)
 *   d_u[B][n] (context dtype), d_flags[B]    outputs
 * Same kernels as irlosc_step_from_q (the fused path when it is on, else front end + step through dense records), with every per-slot
 * input replaced by the caller's pointers; no copies, no host synchronisation, everything enqueued on hip_stream (NULL = the context's
 * stream).  `slot` lends its buffers as the call's scratch: the walk's layout of the coordinates, dense records of the robots the
 * eigen stage gives up on (fused) or of all robots (dense path), and its wrench record.  AFTERWARDS THAT SLOT HOLDS NO RECORDS AND NO
 * JOINT COORDINATES: irlosc_step, irlosc_step_from_q, irlosc_step_resident* and irlosc_download_records on it fail with
 * IRLOSC_ERR_STATE until it is filled again; its targets and sensor feed are not touched.  Like irlosc_step_device the call uses the
 * context's bank-0 scratch (give-up lists, counters, exchange buffer): it must not overlap with other calls on the same context. */
IRLOSC_API int irlosc_step_from_q_device(irlosc_ctx* ctx, int32_t slot, int32_t B, const double* d_qpos, const double* d_qvel,
                                         const void* d_tgt_pose, const void* d_tgt_vel, const double* d_sensordata,
                                         void* d_u, uint32_t* d_flags, void* hip_stream);

/* ---- closed loops on the GPU: a contact-free plant behind the fused step (csrc/osc_plant.hpp) ---------------------------
 * What examples/closed_loop_headless.py does on the host per tick, as one more kernel behind a fused step from joint coordinates:
 *     rhs_j = (ctrl_mask bit j ? u_j : 0) - bias_j - damping qvel_j;   qacc = M^-1 rhs;   qvel += dt qacc;   qpos += dt qvel
 * from the M, bias the step's own walk left in its exchange buffer and the u the step computed, written back into the slot's
 * coordinates (row-major and walk layout alike).  NOT a simulator: no contacts (but the penalty walls of irlosc_set_walls), and joint limits, the gripper's equality rows and a driven gripper only as the penalty rows of irlosc_set_joints.  float64
 * arithmetic whatever the context's dtype (u is read in the context's dtype). */
typedef struct irlosc_plant {
    double dt;               /* > 0, finite */
    double damping;          /* >= 0, finite: joint damping, the same for every joint */
    uint32_t ctrl_mask;      /* bit j: joint j is torque-driven by u_j (bits >= n must be clear) */
    uint32_t reserved;       /* 0 */
} irlosc_plant;
/* After irlosc_set_model (IRLOSC_ERR_STATE before).  A plant that fails the checks above is refused (IRLOSC_ERR_ARG) and the one in
 * force stays.  A later irlosc_set_model clears the plant.  Setting a plant launches nothing and changes no other entry point. */
IRLOSC_API int irlosc_set_plant(irlosc_ctx* ctx, const irlosc_plant* plant);
/* `ticks` (>= 1) dependent ticks on slot `slot`'s B robots, enqueued back to back on the context's stream, one host synchronisation
 * at the end.  A tick is one fused train of one step on bank 0 -- walk, the sensor feed's wrench if the slot has a feed (its readings
 * stay what irlosc_set_sensordata put there; a sensed push of the slot, irlosc_set_pushes, and the force of its walls, irlosc_set_walls, are taken off the wrench computed from them), OSC step, eigen pass, give-up pass -- and behind it the plant kernel.  Targets (target
 * velocities included) are the slot's, gains the context's.  The slot keeps B robots of coordinates, targets and feed; as after
 * every fused step it holds no dense records afterwards.
 *   trace_every > 0 and ee_trace_host != NULL: ee_trace_host[i][B][ndev][7] (double) = the EE poses at the START of tick
 *       i * trace_every, ceil(ticks / trace_every) samples.  The device buffer behind it is bounded (256 MiB, at least one sample):
 *       a longer trace crosses PCIe in chunks, each copy ordered on the stream behind the ticks that filled it.
 *   u_host[B][n] (context dtype, or NULL): the torques of the LAST tick;  flags_any_host[B] (or NULL): the OR of every tick's flags.
 * A robot whose u or qacc is not finite, or whose M has a pivot that is not positive, is FROZEN for that tick (coordinates
 * unchanged) with IRLOSC_FLAG_NONFINITE resp. IRLOSC_FLAG_M_NOT_PD in flags_any; other robots are unaffected.
 * The plant reads the exchange buffer, so the rollout exists where the fused path does: IRLOSC_ERR_STATE with the reason in
 * irlosc_last_error otherwise (no model / plant / gains, a model or context without the fused path, IRLOSC_FUSED=0, exchange buffers
 * that could not be allocated, a slot without coordinates or targets for B robots).  There is no second form. */
IRLOSC_API int irlosc_rollout_from_q(irlosc_ctx* ctx, int32_t slot, int32_t B, int32_t ticks, int32_t trace_every,
                                     double* ee_trace_host, void* u_host, uint32_t* flags_any_host);
/* The slot's joint coordinates as they sit in HBM (uploaded, or advanced by irlosc_rollout_from_q): qpos, qvel [B][n] double, either
 * may be NULL.  IRLOSC_ERR_STATE on a slot that holds coordinates of fewer than B robots (none after irlosc_step_from_q_device lent
 * it).  Synchronous. */
IRLOSC_API int irlosc_download_q(irlosc_ctx* ctx, int32_t slot, int32_t B, double* qpos, double* qvel);

/* ---- ONE WRITER OF THE TARGETS: the program of a slot's rollouts -------------------------------------------------------------
 * Inside a rollout the slot's targets are written by at most one PROGRAM: waypoint paths (irlosc_set_waypoints), a WP / GRIP action
 * list (irlosc_set_action_list), a teleoperation stream (irlosc_set_teleop_stream) or a policy (irlosc_set_policy), never two of them; outside one by
 * irlosc_set_targets.  Targets are written by one entry point at a time:
 *     irlosc_set_targets on the slot (B == 0 too), irlosc_set_model (all slots)        any program ends
 *     irlosc_set_gains (all slots)                                                     a list ends (its gain copy is stale), paths and a stream stay
 *     irlosc_set_waypoints with desc == NULL or all counts 0                           paths end, a list or a stream stays
 *     irlosc_set_action_list with desc == NULL                                         a list ends, paths or a stream stay
 *     irlosc_set_teleop_stream with desc == NULL                                       a stream ends, paths or a list stay
 *     irlosc_set_policy with desc == NULL                                              a policy ends (and episodes set on it), every other program stays
 *     a setter that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE                         nothing changes: the program in force stays, whole
 *     a setter that succeeds                                                           its program replaces whatever was in force
 *     a setter that answers IRLOSC_ERR_HIP (allocation, copy or init launch)           no program of its kind; irlosc_set_waypoints and
 *                                                                                      irlosc_set_teleop_stream: none
 * Uploads of coordinates, records and sensor feeds leave the program alone.  Only irlosc_rollout_from_q runs it (on at most the B
 * robots it was set for: IRLOSC_ERR_STATE beyond); every other step ignores it and leaves its state as it is.  Its tick counts the
 * slot's rollout ticks since its setter and continues across calls of irlosc_rollout_from_q.  Clearing a program leaves the targets
 * as they are.
 * EXTERNAL PUSHES (irlosc_set_pushes) write no targets, so they are no program: they coexist with paths and with a list, and neither
 * ends the other.  What ends them: irlosc_set_pushes with desc == NULL, and irlosc_set_model (the exchange block's entry layout belongs
 * to the model).  Uploads, irlosc_set_targets, irlosc_set_gains and sensor feeds leave them and their tick alone.  Like a program only
 * irlosc_rollout_from_q runs them and advances their tick.
 * COMPLIANT WALLS (irlosc_set_walls) write no targets either: they coexist with paths, a list and pushes, and none ends another.
 *     irlosc_set_walls with desc == NULL, irlosc_set_model (all slots)                 walls end
 *     irlosc_set_walls that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE                 nothing changes: the walls in force stay, whole
 *     irlosc_set_walls that succeeds                                                   its walls replace those in force; state and tick reset
 *     irlosc_set_walls that answers IRLOSC_ERR_HIP                                     no walls
 *     everything else (uploads, targets, gains, feeds, programs, pushes, other steps)  leaves them, their state and their tick alone
 * Only irlosc_rollout_from_q runs them and advances their tick.
 * JOINT ROWS (irlosc_set_joints) write no targets either: they coexist with paths, a list, pushes and walls, and none ends another.
 *     irlosc_set_joints with desc == NULL, irlosc_set_model (all slots)                rows end
 *     irlosc_set_joints that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE                nothing changes: the rows in force stay, whole
 *     irlosc_set_joints that succeeds                                                  its rows replace those in force; state and tick reset
 *     irlosc_set_joints that answers IRLOSC_ERR_HIP                                    no rows
 *     everything else (uploads, targets, gains, feeds, programs, pushes, walls, other steps)  leaves them, their state and their tick alone
 * Only irlosc_rollout_from_q runs them and advances their tick.  An ACTION drive row reads the list in force on the tick it runs: with no
 * list, or one whose active device is not the row's, it is idle and keeps its ctrl -- legal, because lists come and go.
 * EPISODES (irlosc_set_episodes) write targets only where they put a robot back to its start, so they are no program either: they live
 * next to paths or a list, walls and joint rows, but their snapshot and their resets belong to the program and the targets they were set on.
 *     irlosc_set_episodes with desc == NULL, irlosc_set_model (all slots)              episodes end
 *     irlosc_set_targets on the slot (B == 0 too)                                      episodes end: the snapshot is stale
 *     a setter of the slot's program that succeeds, or that ends the program in force
 *     (irlosc_set_waypoints, irlosc_set_action_list, irlosc_set_policy; irlosc_set_gains where it ends a list)   episodes end
 *     irlosc_set_episodes that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE              nothing changes: the episodes in force stay, whole
 *     irlosc_set_episodes that succeeds                                                its episodes replace those in force; state and tick reset
 *     irlosc_set_episodes that answers IRLOSC_ERR_HIP                                  no episodes
 *     irlosc_set_teleop_stream, irlosc_set_pushes on a slot with episodes              REFUSED (IRLOSC_ERR_STATE), as irlosc_set_episodes is on a
 *                                                                                      slot with a stream or with pushes: the reading index and
 *                                                                                      the windows are the slot's ticks, not a robot's
 *     everything else (uploads of coordinates, feeds, gains without a list, walls, joint rows, other steps)  leaves them alone
 * Only irlosc_rollout_from_q and irlosc_rollout_from_q_logged run them and advance their tick.
 * ACTION OBJECTS (irlosc_set_objects, "action objects" below) write no targets and, without loads, act on nothing: they coexist with every
 * program, pushes, walls, joint rows and episodes, and none ends another.  Their LOADS (irlosc_set_object_loads) are a side description of
 * the objects in force -- a carried object's weight on the plant and in the feed -- and end with them:
 *     irlosc_set_object_loads with desc == NULL                                        the loads end; the objects and their state stay
 *     irlosc_set_object_loads that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE          nothing changes: the loads in force stay, whole
 *     irlosc_set_object_loads that succeeds                                            its loads replace those in force; their state and tick reset
 *     irlosc_set_object_loads that answers IRLOSC_ERR_HIP                              no loads, the objects stay
 *     irlosc_set_objects (set or clear, unless refused), irlosc_set_model              the loads end  A list's REFS (irlosc_set_action_refs) name the objects in force:
 *     irlosc_set_objects with desc == NULL, irlosc_set_model (all slots)               objects end, and the list's refs with them
 *     irlosc_set_objects that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE               nothing changes: objects and refs in force stay, whole
 *     irlosc_set_objects that succeeds                                                 its objects replace those in force; state and tick reset; refs end
 *     irlosc_set_objects that answers IRLOSC_ERR_HIP                                   no objects, no refs
 *     whatever ends or replaces the slot's list                                        refs end, objects stay
 *     everything else (uploads, targets, gains, feeds, pushes, walls, joint rows, episodes, other steps)  leaves them, their state and their tick alone
 * Only the two rollout entry points run them and advance their tick; episodes reset a robot's objects with the rest of it.
 * A list's MOTION (irlosc_set_action_motion, "the motion of the list in force" below) is a side description of the list, like its refs:
 * it writes the targets only through the list's own kernel, so the list stays the one writer.
 *     irlosc_set_action_motion with motion == NULL                                     the motion ends, the list stays (and jumps again)
 *     irlosc_set_action_motion that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE         nothing changes: the motion in force stays, whole
 *     irlosc_set_action_motion that succeeds                                           its motion replaces the one in force; its state reset
 *     irlosc_set_action_motion that answers IRLOSC_ERR_HIP                             no motion, the list stays
 *     whatever ends or replaces the slot's list (irlosc_set_action_list included)      the motion ends
 *     everything else (refs, objects, episodes, uploads, feeds, pushes, walls, rows)   leaves it and its state alone; a reset of
 *                                                                                      episodes keeps a robot's draws
 * A policy's GAUSSIAN HEAD (irlosc_set_policy_noise, "a stochastic policy head" below) is a side description of the policy in the same way:
 *     irlosc_set_policy_noise with noise == NULL                                       the head ends, the policy stays (deterministic again)
 *     irlosc_set_policy_noise that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE          nothing changes: the head in force stays, whole
 *     irlosc_set_policy_noise that succeeds                                            its head replaces the one in force; its state reset
 *     irlosc_set_policy_noise that answers IRLOSC_ERR_HIP                              no head, the policy stays
 *     whatever ends or replaces the slot's policy (irlosc_set_policy included)         the head ends
 *     everything else                                                                  leaves it and its state alone; a reset of episodes
 *                                                                                      zeroes a robot's act and logp and keeps its draws
 * A REWARD (irlosc_set_reward, "a reward per tick" below) writes no targets and acts on nothing: it READS other parts -- the targets, a
 * policy's action, the objects and their mates, the feed's wrench -- by name, and none of their setters looks at it.
 *     irlosc_set_reward with desc == NULL, irlosc_set_model (all slots)                the reward ends
 *     irlosc_set_reward that answers IRLOSC_ERR_ARG or IRLOSC_ERR_STATE                nothing changes: the reward in force stays, whole
 *     irlosc_set_reward that succeeds                                                  its reward replaces the one in force; its state reset
 *     irlosc_set_reward that answers IRLOSC_ERR_HIP                                    no reward
 *     a part the reward names ends or shrinks (objects, a policy, the feed, targets)   the reward STAYS, and the next rollout call is
 *                                                                                      refused (IRLOSC_ERR_STATE, with the reason) until the
 *                                                                                      part is back or the reward is set again or ended
 *     everything else                                                                  leaves it and its state alone; a reset of episodes
 *                                                                                      makes a robot's reward state fresh
 * Only the two rollout entry points run it.  Order of use: the parts, then the reward, then (optionally) the episodes. */

/* ---- waypoint paths on the GPU: the rollout's targets cycle like gain_test's (csrc/osc_waypoint.hpp) ----------------------
 * What examples/headless_loops.py::gain_test_loop does on the host per tick, as one more small kernel of a rollout tick, between
 * the give-up pass and the plant.  Robot b, device d with W_d > 0 waypoints and index idx in [0, W_d] (idx == W_d: path finished,
 * loop[d] == 0 only; a finished device is skipped):
 *     e = EE xyz of this tick's walk (double);   t = (double) tgt[b][d][0..2] as stored          -- what the OSC step of this tick saw
 *     d2 = (e0-t0)^2 + (e1-t1)^2 + (e2-t2)^2;    reached = d2 < threshold[d]^2                   -- a NaN anywhere: not reached
 *     if reached:  arrivals += 1;  last_tick = tick;  idx = idx + 1 < W_d ? idx + 1 : (loop[d] ? 0 : W_d)
 *                  tgt[b][d][0..2] = waypoint min(idx, W_d - 1), in the context's dtype          -- the quaternion words stay
 * The reference's order: the index moves after `generate` and is judged on the state `generate` used.  `tick` counts the slot's
 * rollout ticks since irlosc_set_waypoints and continues across calls of irlosc_rollout_from_q.  A robot is judged on its EE position
 * alone: one the plant freezes keeps its place in the path unless a NaN reaches that position. */
#define IRLOSC_MAX_WAYPOINTS 64
typedef struct irlosc_waypoints {
    int32_t count[IRLOSC_MAX_DEV];      /* W_d in [0, IRLOSC_MAX_WAYPOINTS]; 0 = device d keeps the slot's target (devices >= ndev: 0) */
    double threshold[IRLOSC_MAX_DEV];   /* metres; finite and > 0 where count > 0 */
    uint8_t loop[IRLOSC_MAX_DEV];       /* 1: wrap to waypoint 0 (gain_test); 0: finish on the last one */
    int32_t nb;                         /* 1 = one table for the fleet, B = a table per robot */
} irlosc_waypoints;
/* Gives slot `slot`'s B robots their paths: xyz[nb][ndev][Wmax][3] double, Wmax = max count (entries [w >= count[d]] are not read).
 * After irlosc_set_model and irlosc_set_targets for at least B robots on the slot (IRLOSC_ERR_STATE otherwise).  Every argument is
 * checked before anything is touched (IRLOSC_ERR_ARG: a count outside [0, 64], a threshold or listed waypoint that is not finite
 * resp. not > 0, loop not 0 / 1, nb not 1 or B, B < 1; the paths in force stay, whole -- as they do when the call answers
 * IRLOSC_ERR_STATE).  On success: idx = 0, arrivals = 0,
 * last_tick = -1 for every listed pair, tick base 0, and waypoint 0 is written into the xyz of the slot's targets of every listed
 * device.  desc == NULL or all counts 0 clears the slot's paths.  What else ends them, what they end and who runs them: "one writer
 * of the targets" above.  Buffers are allocated by the first use; IRLOSC_ERR_HIP when that fails, and the slot is left without
 * paths.  Synchronous. */
IRLOSC_API int irlosc_set_waypoints(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_waypoints* desc, const double* xyz);
/* index, arrivals, last_tick: each [B][ndev], any may be NULL.  Devices without a list report index -1, arrivals 0, last_tick -1.
 * IRLOSC_ERR_STATE on a slot without paths, or with paths for fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_waypoint_state(irlosc_ctx* ctx, int32_t slot, int32_t B, int32_t* index, uint32_t* arrivals,
                                              int32_t* last_tick);

/* ---- the WP / GRIP action list on the GPU: the insertion demo's fleet loop inside a rollout (csrc/osc_action.hpp) -----------------
 * What action_sequence.py::FleetActionSequenceRunner.tick + after_step do on the host per tick, as one more small kernel of a rollout
 * tick, between the walk (and the sensor feed's wrench) and the first OSC kernel: the target and gain changes it makes are seen by
 * THIS tick's OSC step.  after_step -- the judgement of the state a plant step produced -- is the start of the FOLLOWING tick, because
 * only the next walk has that state's EE pose.  Robot b on tick t since irlosc_set_action_list (a = its action, A = n_actions).  A
 * robot's list starts on the FIRST TICK THAT RUNS IT: tick 0 under rollouts over all B robots of the list, a later tick for a robot that
 * earlier rollouts over fewer robots left out.  On that tick it is not judged, start_xyz is taken and action 0 is entered;
 * finished_tick counts the slot's ticks since irlosc_set_action_list all the same.
 *   1. not b's first tick and a < A:  err = 2-norm of calc_error(ee[active_dev], tgt[b][active_dev] as stored) (osc.py:101-118, all six entries,
 *                        float64);  WP: err <= max_error[a] -> a += 1 (a NaN never advances);  GRIP: grip_left -= 1, <= 0 -> a += 1;
 *                        a == A: finished_tick = t
 *   2. b's first tick:   start_xyz = EE xyz of active_dev
 *   3. a < A, not yet entered:  gripper_force = gripper_force[a];
 *                        WP:   tgt[b][passive_dev] = its EE xyz, with its EE quaternion (passive_hold_orientation) or passive_quat;
 *                              tgt[b][active_dev] = pose[b][a], xyz replaced by start_xyz where xyz_from_start[a];  err = +inf
 *                        GRIP: grip_left = grip_ticks[a]; targets stay
 *   4. a < A and WP:     max_vel0 = max(min_speed[a], min(max_speed[a], kp[a] * err)) into word 9 (max_vel0) of active_dev's gain record
 *                        of robot b, in the SLOT'S OWN gain copy [B][ndev][IRLOSC_GAIN_WORDS] (made from the context's gains by
 *                        irlosc_set_action_list; the context's gains are never written, other slots and entry points see no change).
 *                        max_vel0 persists through GRIP actions and after the list ends.
 * A robot that has finished holds its last targets and gains.  gripper_force is state, as in FleetActionSequenceRunner; it drives a
 * gripper where the slot has an ACTION drive row on active_dev (irlosc_set_joints): on every tick with a non-zero gripper_force the
 * row's ctrl takes it, and gear x ctrl acts on the row's hinge in the plant step of the same tick.  Without such a row no gripper
 * joint is driven. */
#define IRLOSC_MAX_ACTIONS 32
#define IRLOSC_ACTION_WP   0
#define IRLOSC_ACTION_GRIP 1
typedef struct irlosc_action_list {
    int32_t n_actions;                        /* A in [1, IRLOSC_MAX_ACTIONS] */
    int32_t active_dev;                       /* device index (targets order) of the arm that runs the list */
    int32_t passive_dev;                      /* the other arm, or -1: none, nothing of it is written */
    int32_t passive_hold_orientation;         /* 1: a WP gives the passive arm its own EE quaternion; 0: passive_quat */
    double passive_quat[4];                   /* w x y z, finite */
    int32_t nb;                               /* 1 = one pose table for the fleet, B = a table per robot */
    int32_t kind[IRLOSC_MAX_ACTIONS];         /* IRLOSC_ACTION_WP / IRLOSC_ACTION_GRIP */
    int32_t xyz_from_start[IRLOSC_MAX_ACTIONS];   /* WP: 1 = target xyz is the active EE position of the robot's first tick ('start_pos') */
    int32_t grip_ticks[IRLOSC_MAX_ACTIONS];   /* GRIP: >= 1 */
    double kp[IRLOSC_MAX_ACTIONS];            /* WP: finite */
    double max_error[IRLOSC_MAX_ACTIONS];     /* WP: finite */
    double min_speed[IRLOSC_MAX_ACTIONS];     /* WP: finite, <= max_speed */
    double max_speed[IRLOSC_MAX_ACTIONS];
    double gripper_force[IRLOSC_MAX_ACTIONS]; /* finite; state, read by ACTION drive rows (irlosc_set_joints) */
} irlosc_action_list;
/* Gives slot `slot`'s B robots the list: pose[nb][A][7] double (x y z qw qx qy qz; rows of GRIP actions are not read).  Every argument
 * is checked before anything is touched (IRLOSC_ERR_ARG: n_actions outside [1, 32], a kind that is neither, device indices outside
 * [0, ndev) or equal, hold flag / xyz_from_start not 0 / 1, nb not 1 or B, B < 1, a value that is not finite, min_speed > max_speed,
 * grip_ticks < 1, pose NULL; the list in force stays, whole -- as it does when the call answers IRLOSC_ERR_STATE).  After
 * irlosc_set_model, irlosc_set_gains and irlosc_set_targets for at least B robots on the slot (IRLOSC_ERR_STATE otherwise; also when
 * the list has a WP and the gains in force have has_max_vel == 0 for active_dev: the limit would be ignored).  On success the slot
 * has its gain copy (the context's gains broadcast or copied, null_kv with them) and the state is reset: action 0, nothing entered,
 * err +inf, max_vel0 0, gripper_force 0, finished_tick -1, tick base 0.  desc == NULL clears the list.  What else ends it, what it
 * ends and who runs it: "one writer of the targets" above; its rollouts read the slot's gain copy in place of the context's gains,
 * every other step ignores both.  Buffers are allocated by the first use.  IRLOSC_ERR_HIP -- an allocation, a copy or the init launch failed -- is the one error that does NOT keep the list in
 * force: the slot is left WITHOUT a list (its rollouts read the context's gains again; its targets stay as the earlier list last
 * wrote them).  Synchronous. */
IRLOSC_API int irlosc_set_action_list(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_action_list* desc, const double* pose);
/* action, grip_left, finished_tick: int32 [B]; err, max_vel0, gripper_force: double [B]; any may be NULL.  THE STATE IS AS OF THE START
 * OF THE LAST TICK RUN: the judgement of the state the last plant step produced happens on the next tick (a robot whose last step
 * brought it within max_error still reports its WP, and finished_tick is the tick that found it done).  finished_tick: -1 until done.
 * IRLOSC_ERR_STATE on a slot without a list, or with a list for fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_action_state(irlosc_ctx* ctx, int32_t slot, int32_t B, int32_t* action, int32_t* grip_left, double* err,
                                            double* max_vel0, double* gripper_force, int32_t* finished_tick);

/* ---- the MOTION of the list in force: INTERP moves and seeded target noise (csrc/osc_action.hpp, csrc/osc_rng.hpp) ------------------
 * A side description of the list in force, like its refs: irlosc_action_list and its validation are untouched and there is no new
 * kind.  An INTERP action of the reference's action_sequence_configs/iros2022_task.yaml is a WP with steps[a] = N >= 1: its target
 * travels from where the arm is to the goal over N control ticks instead of jumping.  `noise: [mean, std]` on a WP or an INTERP is
 * Gaussian scatter on the goal's position, so that no two demonstrations are alike.  (The reference ships no runner for that file:
 * these semantics are this library's.)  A slot with a motion runs the action kernel's MOTION form; the list's four steps hold, with:
 *   3'. entry of a WP:   the goal is composed as in step 3 (table, start_xyz, refs) and KEPT IN FLOAT64.  An action with noise
 *                        (noise_std[a] > 0 or noise_mean[a] != 0): goal_c += noise_mean[a] + noise_std[a] * z_c for c in x, y, z, every
 *                        product and sum rounded on its own; then draws += 1.  goal is stored, origin = active_dev's EE pose of this
 *                        tick, step = 0.  The entry of a GRIP writes none of the motion's state.
 *       the draw:        (z_0, z_1, z_2) are Box-Muller normals of ONE Philox4x32-10 block: key (seed's low 32 bits, its high 32 bits),
 *                        counter (robot's index in the slot, draws before the increment, a, 0).  The index is the slot's, not a lane's:
 *                        a rollout over fewer robots changes nobody's draws.  u = (2 w0 + 1) / 2^33, r = sqrt(-2 ln u), z_0 = r cos(2 pi
 *                        w1 / 2^32), z_1 = r sin(same); z_2 the cosine branch of (w2, w3).  ln, sin and cos are written out in add,
 *                        multiply, divide and square root (csrc/osc_rng.hpp), so the host repeats every bit
 *                        (irl_control_amd/action_motion.py: normal3).
 *       steps[a] == 0:   tgt[b][active_dev] = goal in the context's dtype, on the entry tick only -- a WP as before.
 *       steps[a] = N:    on the entry tick and on every later tick in this action while step < N:  step += 1, w = step / N.
 *                        step < N:   xyz_c = origin_c + w * (goal_c - origin_c);  the quaternion is an nlerp on the short arc: both ends
 *                                    divided by their norms, the goal's sign flipped where their dot product is negative, the blend
 *                                    qa_c + w * (qb_c - qa_c) divided by its norm.
 *                        step == N:  the seven goal words as composed -- no flip, no renormalisation -- so steps = 1 without noise is
 *                                    a WP bit for bit.
 *   1'. judgement:       err stays the error against the target AS STORED, which is now the moving one, and feeds the limit of step 4
 *                        unchanged.  An INTERP advances only when step == N and err <= max_error[a].
 * All arithmetic above is add, multiply, divide, square root and integer operations, each rounded on its own, in float64 whatever the
 * context's dtype; the targets are rounded to the dtype when they are written.
 * EPISODES: a reset leaves the list as irlosc_set_action_list does -- nothing entered -- so the robot's next tick enters action 0 again,
 * which rewrites goal, origin and step.  draws is deliberately NOT reset: every episode of a robot draws fresh noise. */
typedef struct irlosc_action_motion {
    int32_t  steps[IRLOSC_MAX_ACTIONS];      /* 0: the WP jumps; N in [1, 1 << 20]: INTERP over N ticks.  WP actions only */
    double   noise_mean[IRLOSC_MAX_ACTIONS]; /* finite; metres; WP actions only */
    double   noise_std[IRLOSC_MAX_ACTIONS];  /* finite, >= 0; WP actions only */
    uint64_t seed;
} irlosc_action_motion;
/* Gives the list in force on slot `slot` its motion.  Call it after irlosc_set_action_list, and after irlosc_set_action_refs where refs
 * are used.  draw0: uint32 [B of the list], every robot's draws to start from, or NULL: zeros (continue a robot's sequence of draws in a
 * fresh rollout by passing the draws it has used).  Every argument is checked before anything is touched -- IRLOSC_ERR_ARG: steps < 0
 * or > 1 << 20, a mean that is not finite, a std that is negative or not finite, or steps / mean / std other than 0 on a GRIP action;
 * IRLOSC_ERR_STATE: the slot has no list.  In both cases the motion in force stays, whole.  Entries beyond n_actions are not read.  On
 * success: step 0, draws = draw0, origin and goal 0 for every robot; the list's own state and its tick are left alone (set the motion
 * before the first rollout).  motion == NULL clears it: the list jumps from pose to pose again.  irlosc_set_action_list, and whatever
 * else ends the list, ends the motion ("one writer of the targets" above).  Buffers are allocated by the first use; IRLOSC_ERR_HIP
 * leaves the list in force WITHOUT a motion.  Synchronous. */
IRLOSC_API int irlosc_set_action_motion(irlosc_ctx* ctx, int32_t slot, const irlosc_action_motion* motion, const uint32_t* draw0);
/* step: int32 [B]; draws: uint32 [B]; origin, goal: double [B][7] (x y z qw qx qy qz); any may be NULL.  As of the last tick run.
 * IRLOSC_ERR_STATE on a slot without a list, with a list for fewer than B robots, or whose list has no motion.  Synchronous. */
IRLOSC_API int irlosc_download_action_motion_state(irlosc_ctx* ctx, int32_t slot, int32_t B, int32_t* step, uint32_t* draws,
                                                   double* origin, double* goal);

/* ---- the space-mouse teleoperation stream on the GPU: a recorded session inside a rollout (csrc/osc_teleop.hpp) ------------------
 * What examples/teleop_loops.py::space_mouse_loop does on the host per tick -- SpaceMouse.update_state() integrates the device's rate
 * readings into a 6-DoF plate pose, the arms' targets ride on the plate and the base turns towards it -- as one more small kernel of a
 * rollout tick, where the action list's goes: between the walk (and the sensor feed's wrench) and the first OSC kernel, so THIS tick's
 * OSC step aims at the targets of this tick's reading (the reference: update_state(), then generate(), on one tick).  One stream can
 * drive the whole fleet, or each robot can have its own.  Robot b on tick t, counted in the slot's rollout ticks since
 * irlosc_set_teleop_stream and continuing across calls of irlosc_rollout_from_q; its reading r = readings[.][i], i = loop ? t mod T : t;
 * pose (x y z roll pitch yaw), inc = increment (input_devices/space_mouse.py:30-38):
 *     x += inc * r[0];  y += inc * r[1];  z += inc * r[2]                              -- each product and each sum rounded on its own
 *     yaw = wrap(yaw - inc * r[5]);  pitch = wrap(pitch - inc * r[4]);  roll = wrap(roll + inc * r[3]);  wrap(a) = atan2(sin a, cos a)
 *     q_p = euler2quat(pitch, roll, yaw, axes='rxyz') = qx(pitch) (x) qy(roll) (x) qz(yaw)    -- pitch and roll swapped, as in the reference;
 *           with (cx, sx), (cy, sy), (cz, sz) the cosine and sine of pitch / 2, roll / 2, yaw / 2:
 *           w = cx (cy cz) - sx (sy sz);  x = cx (sy sz) + sx (cy cz);  y = cx (sy cz) - sx (cy sz);  z = cx (cy sz) + sx (sy cz)
 *     RIGID device d:    tgt xyz = p + R(q_p) off_xyz[d]   (R: quat2mat, rows summed left to right);
 *                        tgt quat = q_p (x) off_quat[d]    (Hamilton product, terms left to right; no normalisation, no sign change)
 *     HEADING device d:  h = atan2(y, x) + heading_offset[d];  tgt quat = (cos(h / 2), 0, 0, sin(h / 2));  the xyz words stay
 *     NONE:              the device keeps the slot's target
 * The arithmetic is float64 whatever the context's dtype; targets are stored as casts to it; target velocities are not touched.  The
 * reference reaches the same rotations through mat2euler -> set_abg -> euler2quat: equal up to the quaternion's sign (1e-15), which
 * calc_error's quat2euler does not see.  With loop == 0 the stream ENDS after T ticks: no kernel runs on ticks t >= T, pose and targets
 * stay as tick T - 1 left them, the tick goes on counting.  A robot that a rollout over fewer robots leaves out keeps its pose and its
 * targets and MISSES those readings: the reading index follows the slot's tick, not the robot's.  Nothing of the exchange block is read:
 * a robot the plant has frozen (a NaN coordinate) is steered like every other.
 * Not covered: examples/teleop_loops.py::ps_move_loop.  Its trigger switches ctrlr_dof_abg per tick, which changes k, and a context's
 * layout is fixed when it is created. */
#define IRLOSC_MAX_STREAM_TICKS 16384
#define IRLOSC_TELEOP_NONE    0   /* the device keeps the slot's target */
#define IRLOSC_TELEOP_RIGID   1   /* target pose = plate pose o (off_xyz, off_quat): all seven words written */
#define IRLOSC_TELEOP_HEADING 2   /* quaternion = rotation about world z by atan2(y, x) + heading_offset; xyz words stay */
typedef struct irlosc_teleop_stream {
    int32_t ticks;                         /* T in [1, IRLOSC_MAX_STREAM_TICKS] */
    int32_t nb;                            /* readings: 1 = one stream for the fleet, B = one per robot */
    int32_t nb_origin;                     /* origin: 1 or B */
    int32_t loop;                          /* 1: reading index = tick mod T; 0: the stream ends after T ticks */
    double increment;                      /* finite (the reference: 0.0015) */
    int32_t kind[IRLOSC_MAX_DEV];          /* IRLOSC_TELEOP_*; devices >= ndev: NONE; at least one device not NONE */
    double off_xyz[IRLOSC_MAX_DEV][3];     /* RIGID: finite */
    double off_quat[IRLOSC_MAX_DEV][4];    /* RIGID: w x y z, | |q|^2 - 1 | <= 1e-12 */
    double heading_offset[IRLOSC_MAX_DEV]; /* HEADING: finite */
} irlosc_teleop_stream;
/* Gives slot `slot`'s B robots the stream: readings[nb][T][6] double (x y z roll pitch yaw rates), origin[nb_origin][6] double (the
 * pose before tick 0).  Every argument is checked before anything is touched (IRLOSC_ERR_ARG: ticks outside [1, 16384], an unknown
 * kind or one other than NONE on a device >= ndev, all kinds NONE, nb / nb_origin not 1 or B, loop not 0 / 1, a value that is not
 * finite -- increment, a reading, an origin, a field of a device that reads it --, an off_quat of a RIGID device that is not of unit
 * length, readings or origin NULL, B < 1; the program in force stays, whole -- as it does when the call answers IRLOSC_ERR_STATE).
 * After irlosc_set_model and irlosc_set_targets for at least B robots on the slot (IRLOSC_ERR_STATE otherwise).  On success the stream
 * replaces whatever program was in force, pose = origin and the tick base is 0; NO targets are written: the first tick does that.
 * desc == NULL clears a stream (and leaves paths or a list alone).  What else ends it and who runs it: "one writer of the targets"
 * above; irlosc_set_gains leaves it.  Buffers are allocated by the first use; IRLOSC_ERR_HIP -- an allocation, a copy or the init
 * launch failed -- leaves the slot WITHOUT a program.  Per-robot readings take 48 T bytes of device memory per robot.  Synchronous. */
IRLOSC_API int irlosc_set_teleop_stream(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_teleop_stream* desc, const double* readings,
                                        const double* origin);
/* pose: [B][6] double (x y z roll pitch yaw as the last tick that ran the robot left it; the origin before the first), tick: one int32
 * (the slot's rollout ticks since the setter); either may be NULL.  IRLOSC_ERR_STATE on a slot without a stream, or with a stream for
 * fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_teleop_state(irlosc_ctx* ctx, int32_t slot, int32_t B, double* pose, int32_t* tick);
/* tgt_pose: [B][ndev][7] in the context's dtype: the slot's targets as they sit in HBM -- given by irlosc_set_targets, or written by the
 * program of the slot's rollouts.  Works with or without a program.  IRLOSC_ERR_ARG: tgt_pose NULL; IRLOSC_ERR_STATE on a slot that
 * holds targets for fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_targets(irlosc_ctx* ctx, int32_t slot, int32_t B, void* tgt_pose);

/* ---- a learned policy steers the teleoperation targets: live input inside a rollout (csrc/osc_policy.hpp) -------------------------
 * A POLICY is the fourth kind of program: where a stream replays recorded space-mouse readings, a policy COMPUTES the tick's reading
 * from the tick's observations -- one small ReLU network for the whole fleet, evaluated per robot and tick on the device -- and hands
 * it to the stream's own integration and follower arithmetic (above: "robot b on tick t"), unchanged.  Its kernel runs where the
 * stream's runs: behind the walk, the feed's wrench with every SENSE launch and the object kernel, in front of the first OSC kernel, so
 * THIS tick's OSC step aims at the targets of THIS tick's output.
 * THE OBSERVATION of a robot is the concatenation, in ascending bit order, of the channels `obs` names; every word is cast to float
 * (round to nearest, a double beyond float's range becomes an infinity):
 *     IRLOSC_OBS_QPOS         n        the coordinates this tick's walk read
 *     IRLOSC_OBS_QVEL         n
 *     IRLOSC_OBS_EE_POSE      ndev 7   the walk's EE poses, device-major (x y z qw qx qy qz)
 *     IRLOSC_OBS_TARGETS      ndev 7   the slot's targets as they stand in front of this tick's write (what the tick before aimed at)
 *     IRLOSC_OBS_WRENCH       ndev 6   the feed's wrench behind every SENSE launch of the tick; zeros on a slot without a sensor feed
 *     IRLOSC_OBS_PLATE        6        the plate pose (x y z roll pitch yaw) before this tick's integration
 *     IRLOSC_OBS_OBJECT_POSE  nobj 7   the action objects' poses as this tick's object kernel left them
 * n_in = the sum of the selected widths, 1 <= n_in <= IRLOSC_POLICY_MAX_IN.
 * THE NETWORK: n_layers in [1, IRLOSC_POLICY_MAX_LAYERS] affine layers, ReLU between them, none behind the last; layer l maps
 * in_l -> out_l with in_0 = n_in, out_l = width[l] for l < n_layers - 1 (each in [1, IRLOSC_POLICY_MAX_WIDTH]) and n_out (6 or 7) for
 * the last.  `weights` holds, layer after layer, W[out_l][in_l] row-major (torch.nn.Linear.weight's layout) and then b[out_l].
 * THE ARITHMETIC is float32 and the host can repeat it bit for bit (irl_control_amd/policy.py::mlp).  With in_l padded by zeros to a
 * multiple of 4 and out_l to a multiple of 16 (padding changes no value: fmaf(0, 0, acc) == acc for every acc the chain meets but -0):
 *     acc = b[j];  for i ascending over the padded inputs:  acc = fmaf(W[j][i], x[i], acc)          -- one rounding per step
 *     hidden layer:  x'[j] = acc > 0 ? acc : 0          last layer:  out[j] = acc
 * (the device runs the chains on v_mfma_f32_16x16x4_f32, whose result is this chain).  Then, per robot:
 *     reading r[c] = (double) clamp(out[c]),  c < 6;  clamp(v) = clip > 0 ? (v < -clip ? -clip : v > clip ? clip : v) : v  (in float)
 *     pose and followers' targets from r exactly as a stream's tick takes them from its reading
 *     n_out == 7:  grip = out[6] > 0 ? grip_close : grip_open, stored per robot; the ACTION drive rows (irlosc_set_joints) of device
 *                  grip_dev read it on the same tick exactly where they read an action list's gripper_force
 * A robot whose observation or output holds a word that is not finite KEEPS pose, targets, out and grip on that tick and gets
 * IRLOSC_FLAG_NONFINITE in flags_any; the robots of its wave are not affected.  A robot that a rollout over fewer robots leaves out keeps
 * all of its state.  A policy is never "finished": next to episodes (irlosc_set_episodes accepts it, unlike a stream -- nothing of a
 * policy follows the slot's tick) an episode ends by max_ticks alone, and a reset puts the plate back to the robot's origin and zeroes out and grip. */
#define IRLOSC_POLICY_MAX_IN     192
#define IRLOSC_POLICY_MAX_WIDTH  128
#define IRLOSC_POLICY_MAX_LAYERS 4
#define IRLOSC_OBS_QPOS         1u
#define IRLOSC_OBS_QVEL         2u
#define IRLOSC_OBS_EE_POSE      4u
#define IRLOSC_OBS_TARGETS      8u
#define IRLOSC_OBS_WRENCH      16u
#define IRLOSC_OBS_PLATE       32u
#define IRLOSC_OBS_OBJECT_POSE 64u
typedef struct irlosc_policy {
    uint32_t obs;                          /* OR of IRLOSC_OBS_*: at least one; OBJECT_POSE only on a slot with action objects */
    int32_t n_layers;                      /* [1, IRLOSC_POLICY_MAX_LAYERS] */
    int32_t width[IRLOSC_POLICY_MAX_LAYERS];   /* width[l], l < n_layers - 1: outputs of hidden layer l, [1, IRLOSC_POLICY_MAX_WIDTH]; the others: 0 */
    int32_t n_out;                         /* 6: the reading; 7: and the grip */
    int32_t keep_obs;                      /* 1: the kernel also stores the observation it used ([B][n_in] float: 4 n_in bytes per robot and tick) */
    int32_t grip_dev;                      /* n_out == 7: the device whose ACTION drive rows take the grip, in [0, ndev); else 0 */
    int32_t nb_origin;                     /* origin: 1 or B */
    float clip;                            /* > 0: the six readings are clamped to [-clip, clip]; 0: no clamp; finite, >= 0 */
    int32_t reserved;                      /* 0 */
    double grip_close, grip_open;          /* n_out == 7: finite and not 0; else not read */
    double increment;                      /* the rig, as irlosc_teleop_stream's: finite */
    int32_t kind[IRLOSC_MAX_DEV];          /* IRLOSC_TELEOP_*; devices >= ndev: NONE; at least one device not NONE */
    double off_xyz[IRLOSC_MAX_DEV][3];     /* RIGID: finite */
    double off_quat[IRLOSC_MAX_DEV][4];    /* RIGID: w x y z, | |q|^2 - 1 | <= 1e-12 */
    double heading_offset[IRLOSC_MAX_DEV]; /* HEADING: finite */
} irlosc_policy;
/* Gives slot `slot`'s B robots the policy: weights as above (float), origin[nb_origin][6] double (the plate pose before tick 0).  Every
 * argument is checked before anything is touched (IRLOSC_ERR_ARG: what irlosc_set_teleop_stream refuses of the rig and the origin; obs
 * 0 or with an unknown bit; n_in outside [1, 192]; n_layers, a width or n_out out of range; a width behind the hidden layers that is
 * not 0; keep_obs not 0 / 1; clip negative or not finite; reserved != 0; n_out == 7 with grip_dev outside [0, ndev) or a force that is
 * 0 or not finite; a weight that is not finite; weights or origin NULL; B < 1).  After irlosc_set_model and irlosc_set_targets for at
 * least B robots (IRLOSC_ERR_STATE otherwise, as is IRLOSC_OBS_OBJECT_POSE on a slot without action objects for B robots -- a rollout
 * checks that again: objects come and go).  On ERR_ARG / ERR_STATE the program in force stays, whole.  On success the policy replaces
 * whatever program was in force (and, like every program's setter, ends the slot's episodes), pose = origin, out = 0, grip = 0, the
 * tick base is 0; NO targets are written: the first tick does that.  The setter packs the weights once into the order the kernel's
 * matrix operands are loaded in.  desc == NULL clears a policy and nothing else.  IRLOSC_ERR_HIP leaves the slot WITHOUT a program.
 * Synchronous. */
IRLOSC_API int irlosc_set_policy(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_policy* desc, const float* weights, const double* origin);
/* pose: [B][6] double; out: [B][n_out] float, the network's output BEFORE the clamp, as the last tick that ran the robot left it (0
 * before the first); grip: [B] double; obs: [B][n_in] float, the observation of the last tick that ran the robot (IRLOSC_ERR_STATE if
 * asked for without keep_obs); tick: one int32.  Any may be NULL.  IRLOSC_ERR_STATE on a slot without a policy, or with one for fewer
 * than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_policy_state(irlosc_ctx* ctx, int32_t slot, int32_t B, double* pose, float* out, double* grip, float* obs,
                                            int32_t* tick);

/* ---- a stochastic policy head: a Gaussian drawn on the device, logged with its log-probability (csrc/osc_policy.hpp, csrc/osc_rng.hpp) --
 * A GAUSSIAN HEAD with a state-independent standard deviation on the policy in force: the network's output becomes the MEAN, the action
 * that steers the plate is sampled around it inside the policy kernel, and per robot the device keeps the action taken and its
 * log-probability under the policy that took it -- what a PPO-style learner reads per tick (the log: IRLOSC_LOG_POLICY_OUT,
 * IRLOSC_LOG_POLICY_SAMPLE).  A slot without a head launches exactly the kernels it launched before there was one.
 * THE ARITHMETIC, per robot b on every tick that runs it, which the host can repeat bit for bit (irl_control_amd/policy.py::sample);
 * mean[c] = the network's output (float, unchanged), d = draws[b] at the start of the tick:
 *     eps[c] = z[c & 3] of normal4(seed, b, d, c >> 2, stream 1): Box-Muller on both word pairs of the Philox4x32-10 block with counter
 *              (b, d, c >> 2, 1) under key seed -- z0 = r0 cos, z1 = r0 sin, z2 = r1 cos, z3 = r1 sin, every ln, sin and cos written
 *              out in correctly rounded operations (action_motion.py::normal4).  Two blocks cover 6 or 7 outputs.  The fourth counter
 *              word is a STREAM: an action list's target noise (irlosc_set_action_motion) is stream 0, so the two never meet under one seed
 *     act[c] = std[c] > 0 ? (float)((double) mean[c] + (double) std[c] * eps[c]) : mean[c]
 *              -- the product and the sum rounded on their own in double (no fma), ONE round-to-nearest cast (beyond float's range: an
 *              infinity); an output with std == 0 is deterministic by selection, so a mean of -0 keeps its sign
 *     s = 0;  for c ascending with std[c] > 0:  s = s + eps[c] * eps[c]   (the product rounded, then the sum);   logp = (-0.5 * s) - C
 *     C = sum over the noisy c, ascending, of ln((double) std[c]), + (m / 2) ln 2 pi, m = their number: computed once by the setter on
 *              the host (irlosc_download_policy_noise_state hands it back as logp_const)
 * logp is the density at the UNROUNDED double mean + std eps, not at the float act: recomputing it from act differs by a few 1e-6.
 * EVERYTHING BEHIND THE NETWORK uses act where the deterministic policy uses out: the clamp, the plate and the followers' targets,
 * grip = act[6] > 0 ? grip_close : grip_open, and the finite verdict, which now covers the observation, mean and act.  A robot that is
 * not finite keeps pose, targets, out, grip, act and logp and gets IRLOSC_FLAG_NONFINITE, as before.  `out` keeps its meaning: the
 * network's output before the clamp -- the mean.
 * draws[b] COUNTS TICKS, not successful draws: + 1 (mod 2^32) on every tick that runs robot b, finite or not; a rollout over fewer robots
 * leaves the others' count alone; a reset of episodes zeroes act and logp and KEEPS draws, so every episode explores afresh. */
typedef struct irlosc_policy_noise {
    uint64_t seed;         /* the Philox key */
    int32_t  n_std;        /* must equal n_out of the policy in force (6 or 7) */
    int32_t  reserved;     /* 0 */
    float    std[8];       /* std[c], c < n_std: finite, >= 0, at least one > 0; the others 0 */
} irlosc_policy_noise;
/* Gives the policy in force on slot `slot` the head; draw0: [B of the policy] draws to start from, or NULL = zeros.  Every argument is
 * checked before anything is touched.  IRLOSC_ERR_ARG: n_std other than the policy's n_out, a std that is negative or not finite, all
 * stds 0, a std behind n_std that is not 0, reserved != 0.  IRLOSC_ERR_STATE: the slot has no policy.  On success act = 0, logp = 0,
 * draws = draw0.  noise == NULL ends the head and nothing else.  The lifetime: "a policy's GAUSSIAN HEAD" above.  Synchronous. */
IRLOSC_API int irlosc_set_policy_noise(irlosc_ctx* ctx, int32_t slot, const irlosc_policy_noise* noise, const uint32_t* draw0);
/* act: [B][n_out] float and logp: [B] double as the last tick that ran the robot left them (0 before the first, and behind a reset of
 * episodes); draws: [B] uint32; logp_const: one double, C above.  Any may be NULL.  IRLOSC_ERR_STATE on a slot without a head, or with
 * one for fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_policy_noise_state(irlosc_ctx* ctx, int32_t slot, int32_t B, float* act, double* logp, uint32_t* draws,
                                                  double* logp_const);

/* ---- a reward per tick on the device, and a goal that ends an episode (csrc/osc_reward.hpp) ------------------------------------------
 * What a learner reads next to (observation, action, logp): per tick and robot a REWARD, stated by the caller as a short list of weighted
 * terms, evaluated by one more small kernel of the tick, accumulated per episode -- plain and discounted -- and, with a GOAL, the
 * success signal that ends an episode before its timeout (irlosc_set_episodes: end_on_finish).  The kernel runs behind the give-up pass
 * (u is complete) and directly in front of the log's FRONT launch, so in front of the waypoint cycler and the plant:
 *     r_t = R(the state tick t observed, the action tick t took);   what that action does shows in r_{t+1}.
 * It only reads the tick's state and writes its own.  A slot without a reward enqueues exactly the launches it enqueued before.
 * POINTS -- where a term reads a position and, for ORI, a quaternion (w x y z):
 *     EE d       words ee0[d] .. + 6 of the tick's exchange block: the pose IRLOSC_LOG_EE_POSE logs for device d
 *     TARGET d   the slot's target row of device d as the tick's OSC step read it, widened exactly
 *     OBJECT o   the pose planes of action object o as this tick's object kernel left them
 *     FIXED p    row p of `points`; it has no orientation
 * TERMS -- each yields a double v; float64 whatever the context's dtype, EVERY operation rounded on its own, in the order written, no
 * fma: irl_control_amd/reward.py::reward_tick repeats every bit.
 *     DIST_SQ(a, b)  dx = a_x - b_x, dy, dz likewise;  s = dx dx;  s = s + dy dy;  s = s + dz dz;  v = s
 *     DIST(a, b)     v = sqrt(s)
 *     ORI(a, b)      d = qa_w qb_w;  d = d + qa_x qb_x;  d = d + qa_y qb_y;  d = d + qa_z qb_z;  v = 1 - |d|
 *     ACT_SQ         s = 0;  for c ascending below n_out:  s = s + (double) act[c] (double) act[c];  v = s      -- act of a Gaussian head,
 *                    else the policy's out: what this tick's policy kernel left (a robot it skipped repeats its last one)
 *     U_SQ           s = 0;  for j ascending below n:  s = s + (double) u_j (double) u_j;  v = s      -- the tick's torques behind the give-up pass
 *     FORCE d        x, y, z = words 0..2 of device d's wrench row as the OSC step read it;  s = x x;  s = s + y y;  s = s + z z;  v = sqrt(s)
 *     MATED m        v = mated_tick[m] >= 0 ? 1.0 : 0.0
 *     ONE            v = 1.0
 * THE TICK, for every robot the call runs (fresh values: r = ret = gret = 0, disc = 1, steps = hold = 0, goal_step = -1):
 *     r = 0.0;  for i ascending:  r = r + weight_i v_i          (the product rounded, then the sum)
 *     steps += 1;   ret = ret + r;   gret = gret + disc r;   disc = disc gamma
 *   with a goal (goal_term >= 0), v the goal term's value of this tick:
 *     hold = (goal_cmp == 0 ? v <= goal_value : v >= goal_value) ? hold + 1 : 0          (a NaN compares false)
 *     goal_step = steps, the first time hold >= goal_hold                                 (then it stays until the state is fresh again)
 * A NON-FINITE REWARD IS STORED AS COMPUTED AND SETS NO FLAG: a robot with a NaN coordinate has a NaN r and ret from then on, never
 * reaches a goal, and flags_any is what it is without a reward.
 * EPISODES: with a reward in force that has a goal, and end_on_finish, a robot's episode is also FINISHED on a tick with goal_step >= 0
 * -- for every program kind, a policy and none included -- and an episode that ends with goal_step >= 0 (finished or timed out) carries
 * IRLOSC_EPISODE_GOAL in its outcome.  On the ending tick (ret, gret) go into the reward's own ring of IRLOSC_MAX_EPISODE_RECORDS
 * entries, entry count mod records beside the episode's record, and a reset makes the reward state fresh.  A PARKED robot goes on
 * accumulating: its records are what count.
 * NOT OFFERED: exp / tanh shaping (the host cannot repeat them bit for bit: the policy's own rule); per-episode variants of `points`;
 * a value head. */
#define IRLOSC_MAX_REWARD_TERMS  8
#define IRLOSC_MAX_REWARD_POINTS 8
#define IRLOSC_REWARD_EE      0      /* point kinds */
#define IRLOSC_REWARD_TARGET  1
#define IRLOSC_REWARD_OBJECT  2
#define IRLOSC_REWARD_FIXED   3
#define IRLOSC_REWARD_DIST_SQ 0      /* term kinds */
#define IRLOSC_REWARD_DIST    1
#define IRLOSC_REWARD_ORI     2
#define IRLOSC_REWARD_ACT_SQ  3
#define IRLOSC_REWARD_U_SQ    4
#define IRLOSC_REWARD_FORCE   5
#define IRLOSC_REWARD_MATED   6
#define IRLOSC_REWARD_ONE     7
typedef struct irlosc_reward {
    int32_t n_terms;                             /* in [1, IRLOSC_MAX_REWARD_TERMS] */
    int32_t n_points;                            /* P in [0, IRLOSC_MAX_REWARD_POINTS] */
    int32_t points_per_robot;                    /* 0: one set of P points for the fleet, 1: a set per robot */
    int32_t goal_term;                           /* -1: no goal; else the term in [0, n_terms) whose value the goal compares */
    int32_t goal_cmp;                            /* 0: v <= goal_value, 1: v >= goal_value */
    int32_t goal_hold;                           /* H >= 1: consecutive ticks the comparison has to hold (1 without a goal) */
    int32_t kind[IRLOSC_MAX_REWARD_TERMS];       /* IRLOSC_REWARD_DIST_SQ .. IRLOSC_REWARD_ONE; entries >= n_terms: 0, as in the arrays below */
    int32_t a_kind[IRLOSC_MAX_REWARD_TERMS];     /* DIST_SQ, DIST, ORI: point a's kind; every other term: 0 */
    int32_t a_index[IRLOSC_MAX_REWARD_TERMS];    /* ... and its device, object or row of `points`; FORCE: the device; MATED: the mate; else 0 */
    int32_t b_kind[IRLOSC_MAX_REWARD_TERMS];     /* DIST_SQ, DIST, ORI: point b; every other term: 0 */
    int32_t b_index[IRLOSC_MAX_REWARD_TERMS];
    int32_t reserved[2];                         /* 0 */
    double  weight[IRLOSC_MAX_REWARD_TERMS];     /* finite */
    double  gamma;                               /* finite, in [0, 1] */
    double  goal_value;                          /* finite (0 without a goal) */
} irlosc_reward;
/* Gives slot `slot`'s B robots the reward; points: [points_per_robot ? B : 1][P][3] double (NULL with P == 0).  Every argument is checked
 * before anything is touched; after a refusal the slot is exactly as it was, the reward in force and its state included.
 *   IRLOSC_ERR_ARG    a field outside its range above; B < 1; a weight, gamma, point or goal_value that is not finite; a kind that does
 *                     not exist; an index outside the context's devices, IRLOSC_MAX_OBJECTS, IRLOSC_MAX_MATES or the P points; ORI on a FIXED point; a
 *                     field of a term that does not read it, or of a term >= n_terms, that is not 0; goal_term outside [-1, n_terms);
 *                     goal_cmp other than 0, 1; goal_hold < 1; points NULL with P > 0; reserved != 0
 *   IRLOSC_ERR_STATE  a reference to a part the slot does not have for B robots: no model, or a context whose n is not the rollout's;
 *                     targets for fewer than B robots (asked of every reward: the rollout needs them); OBJECT o with o >= the slot's
 *                     objects; MATED m with m >= its mates; ACT_SQ without a policy; FORCE d without a sensor feed, or on a device the
 *                     feed has no force sensor for; episodes in force for more than B robots (their resets write the reward's state)
 * The two rollout entry points make the SAME state check on every call: a part that was ended under a reward that names it is refused
 * there with the reason, and the reward stays.  On success the state is fresh (the values above) and the reward's ring is not touched:
 * the download masks what no episode of the running count has written.  desc == NULL ends the reward; what else ends it: "one writer of the
 * targets" above.  Buffers are allocated by the first use; IRLOSC_ERR_HIP leaves the slot without a reward.  Synchronous. */
IRLOSC_API int irlosc_set_reward(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_reward* desc, const double* points);
/* r, ret, gret: [B] double -- the last tick's reward and the running episode's sums; steps, hold, goal_step: [B] int32; records:
 * [B][IRLOSC_MAX_EPISODE_RECORDS][2] double, (ret, gret) of ended episodes, entry e of a robot being its episode e' = the largest
 * e' < count with e' mod records == e, as irlosc_download_episode_state has them -- and ZERO for an entry that no episode ended under this
 * reward has written (entries >= records or >= count, episodes that ended before the reward was set, a robot the episodes do not cover, a slot without episodes).  Any may be
 * NULL.  IRLOSC_ERR_STATE on a slot without a reward, or with one for fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_reward_state(irlosc_ctx* ctx, int32_t slot, int32_t B, double* r, double* ret, double* gret, int32_t* steps,
                                            int32_t* hold, int32_t* goal_step, double* records);

/* ---- external pushes on the plant, sensed by the F/T feed: admit_test / force_test inside a rollout (csrc/osc_push.hpp) ------------
 * What examples/headless_loops.py::admit_test_loop does on the host -- xfrc_applied on a gripper body during a window of ticks, the
 * F/T sensors reading the reaction after sim.step() (fakesim.ToyDynamics), the next `generate` yielding to it -- as up to two more
 * small launches of a rollout tick.  The force is prescribed by the caller, as in the reference; there is no contact model.
 * Robot b on tick t, counted in the slot's rollout ticks since irlosc_set_pushes (it continues across calls of irlosc_rollout_from_q):
 *     W_d(t) = the sum, in ascending p, of wrench[b][p] over the pushes with dev[p] == d and tick0[p] <= t < tick1[p]: float64, the
 *              first term taken as it is, every add rounded on its own.  W_d^apply takes the pushes with apply[p], W_d^sense those
 *              with sense[p].
 *   APPLY, behind the give-up pass and the waypoint cycler, in front of the plant kernel: for every device d with a non-empty
 *     W_d^apply(t), in ascending d, and every hinge i above that device's EE body
 *         bias_i <- bias_i - sum_{c = 0..5} J_d[c][i] W_d^apply(t)[c]          (an fma chain in ascending c)
 *     in place on the tick's exchange block, so that the unchanged plant integrates M^-1 (u - bias - damping qvel + sum_d J_d^T W_d).
 *     J_d is the EE body's Jacobian the walk left in the block (jacp rows, then jacr rows, at the body's FRAME ORIGIN), all six rows
 *     whatever rows the layout controls.  The force therefore acts at the EE body's frame origin -- the point the controller
 *     controls -- and the torque is a pure couple.  MuJoCo's xfrc_applied acts at the body's centre of mass, and the reference demo
 *     pushes a gripper body below the EE: this is the contact-free stand-in, not MuJoCo.  Two devices that name one EE body sum.
 *   SENSE, between the sensor feed's wrench kernel and every kernel that reads the wrench (action kernel, OSC kernels, give-up pass):
 *     the reference reads the sensors after the step that felt the push, so the OSC step of tick t sees the push of tick t - 1.  On
 *     tick t >= 1, for every device d with a non-empty W_d^sense(t - 1)
 *         wrench[b][d][c] <- (T)((double)wrench[b][d][c] - W_d^sense(t - 1)[c])          (T: the context's dtype)
 *     -- ToyDynamics' sign ("the reaction": s0 - xfrc_applied), taken in the world frame.  Only where the slot has a sensor feed and
 *     the device a sensor; elsewhere `sense` changes nothing, as a feed changes nothing without IRLOSC_ADMITTANCE.  The slot's record
 *     wrench is never written.
 * A tick on which nothing is applied and nothing is sensed launches exactly the kernels a slot without pushes launches: the host
 * knows the tick, the active sets are kernel arguments, there is no device-side tick state. */
#define IRLOSC_MAX_PUSHES 8
typedef struct irlosc_pushes {
    int32_t n_pushes;                       /* P in [1, IRLOSC_MAX_PUSHES] */
    int32_t nb;                             /* 1 = one wrench table for the fleet, B = a table per robot */
    int32_t dev[IRLOSC_MAX_PUSHES];         /* target device (targets order) whose EE body is pushed */
    int32_t tick0[IRLOSC_MAX_PUSHES];       /* active on ticks t with tick0 <= t < tick1; 0 <= tick0 < tick1 */
    int32_t tick1[IRLOSC_MAX_PUSHES];
    uint8_t apply[IRLOSC_MAX_PUSHES];       /* 1: acts on the plant */
    uint8_t sense[IRLOSC_MAX_PUSHES];       /* 1: appears in the F/T wrench, one tick later */
} irlosc_pushes;
/* Gives slot `slot`'s B robots their pushes: wrench[nb][P][6] double, world frame, fx fy fz tx ty tz; tick base 0.  After
 * irlosc_set_model (IRLOSC_ERR_STATE before).  Every argument is checked before anything is touched (IRLOSC_ERR_ARG: P outside [1, 8],
 * dev outside [0, ndev), a window that is not 0 <= tick0 < tick1, apply or sense not 0 / 1 or both 0, nb not 1 or B, B < 1, wrench
 * NULL or holding a value that is not finite; the pushes in force stay, whole).  desc == NULL clears the slot's pushes; what else ends
 * them and who runs them: "one writer of the targets" above.  A rollout over more robots than the pushes cover answers
 * IRLOSC_ERR_STATE.  The table is allocated by the first use and kept; IRLOSC_ERR_HIP -- the allocation or the copy failed -- leaves the
 * slot without pushes.  Synchronous. */
IRLOSC_API int irlosc_set_pushes(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_pushes* desc, const double* wrench);

/* ---- compliant walls on EE bodies, sensed by the F/T feed: force_test's wall inside a rollout (csrc/osc_wall.hpp) ------------------
 * In the reference's force_test the left arm walks a line of waypoints into a wall whose geom has solref="-900 -20": a direct spring
 * (900) and damper (20).  Here a wall is a half-space with stiffness and damping, and the EE a sphere of radius r around the EE body's
 * FRAME ORIGIN -- the point the controller controls.  The force is computed on the device, per robot and per tick, from the state the
 * rollout itself produced: a closed loop.  It is NOT MuJoCo's soft constraint: no friction, no geometry beyond planes, one contact point.
 * Robot b on tick t, counted in the slot's rollout ticks since irlosc_set_walls (it continues across calls of irlosc_rollout_from_q),
 * wall w on device d, table row  nx ny nz off r k c 0  (n a unit vector of the world frame, n.x >= off the free side):
 *     x   = the EE xyz of this tick's walk;   v_c = sum_i J_d[c][i] qvel_i, c = 0..2, over the hinges above the EE body in ascending i
 *           (J_d: the EE body's jacp rows at its frame origin, qvel as this tick's walk read it)
 *     g   = r - ((n0 x0 + n1 x1 + n2 x2) - off)        s = n0 v0 + n1 v1 + n2 v2        f = k g - c s
 *     F_w = (g > 0 && f > 0) ? f n : 0
 *     F_d(t) = the sum of F_w over the device's walls in ascending w, the first term taken as it is.
 *   Float64 whatever the context's dtype; every product, add and subtract rounded on its own, sums left to right as written (the host
 *   can repeat it: irl_control_amd/walls.py).  A wall never pulls.  A NaN anywhere gives no contact and no force.
 *   APPLY, behind the give-up pass, the waypoint cycler and the pushes' APPLY, in front of the plant kernel: for devices in ascending d
 *     and every hinge i above the EE body   bias_i <- fma(-J_d[2][i], F2, fma(-J_d[1][i], F1, fma(-J_d[0][i], F0, bias_i)))   in place
 *     on the tick's exchange block.  A robot whose F_d is all zero has its bias left as it is.  F_d(t) goes into the per-robot state,
 *     zeros included.
 *   SENSE, between the pushes' SENSE and the action kernel, on every tick t >= 1, where the slot has a sensor feed and the device a
 *     sensor:   wrench[b][d][c] <- (T)((double)wrench[b][d][c] - F_d(t - 1)[c]), c = 0..2; the torque words are untouched.  F_d(t - 1)
 *     is the stored force of the last tick that ran robot b.
 * State per robot and device, reset by the setter: force[3] (what the last tick applied), max_depth (the largest g > 0 seen, or 0),
 * contact_ticks (ticks on which a wall of the device had g > 0), first_tick (the first such tick, or -1).
 * A slot without walls launches exactly the kernels it launched before. */
#define IRLOSC_MAX_WALLS 8
typedef struct irlosc_walls {
    int32_t n_walls;                        /* W in [1, IRLOSC_MAX_WALLS] */
    int32_t nb;                             /* 1 = one table for the fleet, B = a table per robot */
    int32_t dev[IRLOSC_MAX_WALLS];          /* target device (targets order) whose EE body the wall acts on */
} irlosc_walls;
/* Gives slot `slot`'s B robots their walls: table[nb][W][8] double, rows  nx ny nz off r k c 0.  After irlosc_set_model (IRLOSC_ERR_STATE
 * before).  Every argument is checked before anything is touched (IRLOSC_ERR_ARG: W outside [1, 8], dev outside [0, ndev), nb not 1 or
 * B, B < 1, table NULL or holding a value that is not finite, | |n|^2 - 1 | > 1e-12, r, k or c < 0; the walls in force stay, whole).
 * desc == NULL clears the slot's walls; what else ends them and who runs them: "one writer of the targets" above.  A rollout over more
 * robots than the walls cover answers IRLOSC_ERR_STATE.  Table and state are allocated by the first use and kept; IRLOSC_ERR_HIP -- an
 * allocation or a copy failed -- leaves the slot without walls.  Synchronous. */
IRLOSC_API int irlosc_set_walls(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_walls* desc, const double* table);
/* The walls' per-robot state of the slot's first B robots: force[B][ndev][3], max_depth[B][ndev] (double), contact_ticks[B][ndev],
 * first_tick[B][ndev] (int32); any may be NULL.  IRLOSC_ERR_STATE: the slot has no walls, or they cover fewer than B robots.
 * Synchronous. */
IRLOSC_API int irlosc_download_wall_state(irlosc_ctx* ctx, int32_t slot, int32_t B, double* force, double* max_depth,
                                          int32_t* contact_ticks, int32_t* first_tick);

/* ---- joint rows: range stops, the gripper's equality rows and a driven gripper inside a rollout (csrc/osc_joint.hpp) ---------------
 * Every hinge of the Dual-UR5 scene but the stand is limited, ten <equality><joint polycoef> rows tie each Robotiq finger linkage to its
 * driven knuckle, and insertion_task.py::send_forces writes the gripper force into the motors on the two driven knuckles.  Here each is a
 * ROW: a torque on one or two hinges computed on the device, per robot and per tick, from those hinges' own coordinates -- explicit
 * penalties, NOT MuJoCo's soft-constraint solver, and no friction loss.  Robot b on a tick of irlosc_rollout_from_q, q / qd the
 * coordinates at the start of the tick, row r with hinges a (and b) and table row t[8]:
 *   IRLOSC_JOINT_LIMIT   t = lo hi k c 0 0 0 0     g_lo = lo - q_a, f_lo = k g_lo - c qd_a, t_lo = (g_lo > 0 && f_lo > 0) ? f_lo : 0
 *                                                  g_hi = q_a - hi, f_hi = k g_hi + c qd_a, t_hi = (g_hi > 0 && f_hi > 0) ? f_hi : 0
 *                        tau_a += t_lo - t_hi.   A stop never pulls; a NaN gives no contact and no force.
 *   IRLOSC_JOINT_COUPLE  t = a0 a1 qa0 qb0 k c 0 0   hinge a is MuJoCo's joint1, the DEPENDENT y, hinge b its joint2, the x (linear
 *                        polycoef only).  e = (q_a - qa0) - (a0 + a1 (q_b - qb0)), de = qd_a - a1 qd_b, f = k e + c de;
 *                        tau_a -= f, tau_b += a1 f.  An f (or a1 f) that is not finite contributes nothing.  The joint1 = y reading
 *                        follows MuJoCo's documentation; it has NOT been compared with MuJoCo on this project (MuJoCo is not installed).
 *   IRLOSC_JOINT_DRIVE   t = gear value 0 0 0 0 0 0   source IRLOSC_JOINT_SRC_CONST: ctrl = value (per robot with a per-robot table).
 *                        IRLOSC_JOINT_SRC_ACTION: ctrl is per-robot state, 0 after the setter, held across ticks; on a tick where the
 *                        slot has an action list in force whose active_dev is the row's dev[r] and robot b's gripper_force state is
 *                        non-zero, ctrl = gripper_force (the reference's `if gripper_force: ctrl[idx] = gripper_force`: a later action
 *                        with force 0.0 keeps the grip).  The action kernel has run on the tick already, so a GRIP entered on tick t
 *                        drives the plant step of tick t.  tau_a += gear ctrl; a ctrl or product that is not finite contributes nothing.
 * tau_j sums the contributions to hinge j in ASCENDING ROW INDEX, the first taken as it is.  Float64 whatever the context's dtype; every
 * product, add and subtract rounded on its own, nothing contracted (the host can repeat it: irl_control_amd/joints.py).  Then, behind the
 * give-up pass, the waypoint cycler, the pushes' APPLY and the walls' APPLY and directly in front of the plant kernel, for every hinge
 * with tau_j != 0:  bias_j <- bias_j - tau_j  in place on the tick's exchange block, so the plant integrates
 * M^-1 (u - bias - damping qvel + tau).  The F/T feed's wrench does NOT see these forces: they act inside the gripper or at arm hinges,
 * not at the site frame.
 * State per robot, reset by the setter: tau[n] (what the last tick applied, zeros included); per row max_violation (the largest g > 0
 * of a LIMIT or |e| of a COUPLE seen, 0 for a DRIVE), active_ticks (ticks with a non-zero contribution of the row), ctrl (DRIVE rows,
 * else 0).  A slot without joint rows launches exactly the kernels it launched before. */
#define IRLOSC_MAX_JOINT_ROWS 48
#define IRLOSC_JOINT_LIMIT  0
#define IRLOSC_JOINT_COUPLE 1
#define IRLOSC_JOINT_DRIVE  2
#define IRLOSC_JOINT_SRC_CONST  0
#define IRLOSC_JOINT_SRC_ACTION 1
typedef struct irlosc_joint_rows {
    int32_t n_rows;                              /* R in [1, IRLOSC_MAX_JOINT_ROWS] */
    int32_t per_robot;                           /* 0 = one table for the fleet, 1 = a table per robot */
    int32_t kind[IRLOSC_MAX_JOINT_ROWS];         /* IRLOSC_JOINT_LIMIT / _COUPLE / _DRIVE */
    int32_t joint_a[IRLOSC_MAX_JOINT_ROWS];      /* hinge index in [0, n) */
    int32_t joint_b[IRLOSC_MAX_JOINT_ROWS];      /* COUPLE: the other hinge, != joint_a; else not read */
    int32_t source[IRLOSC_MAX_JOINT_ROWS];       /* DRIVE: IRLOSC_JOINT_SRC_CONST / _ACTION; else not read */
    int32_t dev[IRLOSC_MAX_JOINT_ROWS];          /* ACTION drive: the device (targets order) whose list drives it; else not read */
} irlosc_joint_rows;
/* Gives slot `slot`'s B robots their joint rows: table[per_robot ? B : 1][R][8] double.  After irlosc_set_model (IRLOSC_ERR_STATE
 * before).  Every argument is checked before anything is touched (IRLOSC_ERR_ARG: R outside [1, 48], per_robot not 0 / 1, B < 1, an
 * unknown kind or source, a hinge index outside [0, n), joint_a == joint_b on a COUPLE, dev of an ACTION drive outside [0, ndev), table
 * NULL or holding a value that is not finite, lo >= hi, k or c < 0; the rows in force stay, whole).  desc == NULL clears the slot's
 * rows; what else ends them and who runs them: "one writer of the targets" above.  A rollout over more robots than the rows cover
 * answers IRLOSC_ERR_STATE.  Table and state are allocated by the first use and kept; IRLOSC_ERR_HIP -- an allocation or a copy failed
 * -- leaves the slot without rows.  Synchronous. */
IRLOSC_API int irlosc_set_joints(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_joint_rows* desc, const double* table);
/* The rows' per-robot state of the slot's first B robots: tau[B][n], max_violation[B][R] (double), active_ticks[B][R] (int32),
 * ctrl[B][R] (double); any may be NULL.  IRLOSC_ERR_STATE: the slot has no joint rows, or they cover fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_joint_state(irlosc_ctx* ctx, int32_t slot, int32_t B, double* tau, double* max_violation,
                                           int32_t* active_ticks, double* ctrl);

/* ---- the episode log: every logged tick's observations and torques, gathered on the GPU (csrc/osc_log.hpp) -------------------------
 * irlosc_rollout_from_q hands back the EE poses and nothing else per tick.  A LOG hands back, per logged tick and per logged robot, the
 * channels the caller picks -- the (observation, action) pairs a policy is trained from -- without cutting the rollout into one-tick
 * calls.  Everything is a double; widening the float32 words of a float32 context (u, targets, wrench) and the uint32 flags is exact,
 * and the host recovers the original bits by casting back.
 *   FRONT channels, gathered directly behind the give-up pass and in front of the waypoint cycler -- the state the OSC step used, the
 *     targets and the wrench it saw, the torques it produced.  A list's or a stream's targets of the tick are in the sample (they are
 *     written in front of the OSC step); a waypoint that the cycler advances on this tick shows up in the next sample.
 *   BACK channels (WALL_FORCE, JOINT_TAU), gathered behind the joint rows and directly in front of the plant: the `force` and `tau` that
 *     irlosc_download_wall_state / irlosc_download_joint_state would read behind this tick.
 * The log only reads: coordinates, torques, flags, programs, pushes, walls and rows of a logged rollout are bit for bit those of the
 * unlogged one, all tick counts continue as there, and the order of a tick's launches (pushes, then walls, then loads, then joint rows on one bias
 * entry) is unchanged.  A rollout without a log launches exactly the kernels it launched before. */
#define IRLOSC_LOG_QPOS        1u   /* [R][n]        coordinates at the START of the tick: what the tick's walk read            */
#define IRLOSC_LOG_QVEL        2u   /* [R][n]                                                                                    */
#define IRLOSC_LOG_EE_POSE     4u   /* [R][ndev][7]  the walk's EE poses: the words irlosc_rollout_from_q's ee_trace carries     */
#define IRLOSC_LOG_TARGETS     8u   /* [R][ndev][7]  as the tick's OSC step read them, widened to double                         */
#define IRLOSC_LOG_WRENCH     16u   /* [R][ndev][6]  the feed's wrench as the OSC step read it (after every SENSE), widened      */
#define IRLOSC_LOG_U          32u   /* [R][n]        the tick's torques (give-up pass included), widened                         */
#define IRLOSC_LOG_FLAGS      64u   /* [R][1]        the step's flag word of the tick as a double (not what the plant adds)      */
#define IRLOSC_LOG_WALL_FORCE 128u  /* [R][ndev][3]  F_d(t) the walls applied on this tick                                       */
#define IRLOSC_LOG_JOINT_TAU  256u  /* [R][n]        tau the joint rows applied on this tick                                     */
#define IRLOSC_LOG_OBJECT_POSE 512u /* [R][nobj][8]  FRONT: the action objects as this tick's object kernel left them: x y z qw qx qy qz
                                       and the holder (-1 = free, else the gripper) as a double.  Only on a slot with action objects
                                       (irlosc_set_objects); elsewhere the bit is unknown: irlosc_log_layout_objects, below          */
#define IRLOSC_LOG_POLICY_OUT    1024u /* [R][n_out]     FRONT: the network's output of this tick (with a Gaussian head: the mean), widened
                                          to double.  Only on a slot with a policy; elsewhere the bit is unknown                        */
#define IRLOSC_LOG_POLICY_SAMPLE 2048u /* [R][n_out + 1] FRONT: act[0 .. n_out) of this tick, widened, then logp.  Only on a slot whose
                                          policy has a Gaussian head (irlosc_set_policy_noise); elsewhere the bit is unknown.  Both show
                                          what this tick's policy kernel left: a robot it skipped (not finite) repeats its last sample */
#define IRLOSC_LOG_REWARD      4096u   /* [R][4]         FRONT: r, ret, steps, goal (goal_step >= 0 ? 1 : 0) as this tick's reward kernel left
                                          them, the last two as doubles.  Only on a slot with a reward (irlosc_set_reward); elsewhere the
                                          bit is unknown: irlosc_log_layout_reward, below                                                */
typedef struct irlosc_log {
    uint32_t channels;      /* OR of the above, not 0, no other bit */
    int32_t  every;         /* >= 1: ticks 0, every, 2 every, ... of THIS call are logged (as trace_every counts) */
    int32_t  n_robots;      /* R: 0 or B with robots == NULL (all B), else the length of robots[] in [1, B] */
    int32_t  reserved;      /* 0 */
    uint64_t buffer_bytes;  /* device ring, 0 = 256 MiB; else it must hold at least two samples */
} irlosc_log;
/* A SAMPLE is the concatenation, in ascending bit order, of the asked channels' planes, each a dense row-major [R][w] array of doubles
 * (channel-major on purpose: a block's 64 robots own 64 w consecutive doubles of a plane, so the kernel's stores are coalesced tiles).
 * Context-free: offset[i] = where the plane of channel bit i starts inside a sample, in doubles (-1 for a channel not asked for), and
 * *sample_words = the sample's size.  IRLOSC_ERR_ARG: channels 0 or with an unknown bit, R < 1, n outside [1, IRLOSC_MAX_N], ndev
 * outside [1, IRLOSC_MAX_DEV], offset or sample_words NULL. */
IRLOSC_API int irlosc_log_layout(int32_t n, int32_t ndev, uint32_t channels, int32_t R, int64_t offset[9], int64_t* sample_words);
/* The same for a slot with nobj action objects (nobj in [0, IRLOSC_MAX_OBJECTS]): ten offsets, the tenth IRLOSC_LOG_OBJECT_POSE's plane
 * [R][nobj][8].  With nobj == 0 that bit is unknown, as it is to irlosc_log_layout, and the first nine offsets are irlosc_log_layout's. */
IRLOSC_API int irlosc_log_layout_objects(int32_t n, int32_t ndev, int32_t nobj, uint32_t channels, int32_t R, int64_t offset[10],
                                         int64_t* sample_words);
/* The same for a slot whose policy has n_out outputs (6 or 7; 0: no policy) and, with sampled == 1, a Gaussian head: twelve offsets, the
 * eleventh IRLOSC_LOG_POLICY_OUT's plane [R][n_out], the twelfth IRLOSC_LOG_POLICY_SAMPLE's [R][n_out + 1].  With n_out == 0 both bits
 * are unknown and the first ten offsets are irlosc_log_layout_objects'; with sampled == 0 IRLOSC_LOG_POLICY_SAMPLE is unknown.
 * IRLOSC_ERR_ARG also for an n_out other than 0, 6, 7 and a sampled other than 0, 1. */
IRLOSC_API int irlosc_log_layout_policy(int32_t n, int32_t ndev, int32_t nobj, int32_t n_out, int32_t sampled, uint32_t channels, int32_t R,
                                        int64_t offset[12], int64_t* sample_words);
/* The same for a slot that, with rewarded == 1, has a reward: thirteen offsets, the thirteenth IRLOSC_LOG_REWARD's plane [R][4].  With
 * rewarded == 0 that bit is unknown and the first twelve offsets are irlosc_log_layout_policy's (the three functions above keep refusing
 * it).  IRLOSC_ERR_ARG also for a rewarded other than 0, 1. */
IRLOSC_API int irlosc_log_layout_reward(int32_t n, int32_t ndev, int32_t nobj, int32_t n_out, int32_t sampled, int32_t rewarded,
                                        uint32_t channels, int32_t R, int64_t offset[13], int64_t* sample_words);
/* irlosc_rollout_from_q with a log in place of the EE trace: log_host[ceil(ticks / every)][sample_words] (double), one sample per logged
 * tick of the R robots of `robots` (strictly ascending, in [0, B); NULL: all B).  log == NULL is
 * irlosc_rollout_from_q(ctx, slot, B, ticks, 0, NULL, u_host, flags_any_host); robots and log_host are not read then.
 * The samples are gathered into a device ring the context owns (allocated by the first use, regrown on demand; with buffer_bytes == 0
 * it is 256 MiB, or two samples where those are larger).  The ring has two halves of whole samples, and a half holds what drains in
 * one piece -- 32 MiB, or one sample where that is larger.  A full half, and the last one, crosses PCIe on a stream of its own into a
 * pinned block while the following ticks fill the other half on the context's stream; the host copies a pinned block into log_host
 * when it needs the block again, and at the end.  Ticks keep running while a half is on the link; the rollout waits only where a half
 * would be refilled before it has left.
 * Every argument is checked before anything is enqueued, sizes in 64 bits; after a refusal the slot is exactly as it was: no tick ran.
 *   IRLOSC_ERR_ARG    what irlosc_log_layout_reward refuses for the slot's action objects, policy, head and reward (IRLOSC_LOG_REWARD on
 *                     a slot without a reward is an unknown bit; none of them: what
 *                     irlosc_log_layout refuses, so IRLOSC_LOG_OBJECT_POSE on a slot without objects, IRLOSC_LOG_POLICY_OUT on one without
 *                     a policy and IRLOSC_LOG_POLICY_SAMPLE on one without a Gaussian head are unknown bits); every < 1; reserved != 0; robots == NULL with n_robots not 0 or B; robots given with
 *                     n_robots outside [1, B], not strictly ascending or outside [0, B); log_host NULL; a buffer_bytes != 0 that
 *                     holds fewer than two samples
 *   IRLOSC_ERR_STATE  what irlosc_rollout_from_q refuses; IRLOSC_LOG_WRENCH on a slot without a sensor feed; IRLOSC_LOG_WALL_FORCE on a
 *                     slot without walls; IRLOSC_LOG_JOINT_TAU on a slot without joint rows (each covers B robots, as every rollout asks)
 * A robot that is frozen on a tick is logged like any other: its coordinates repeat, its u and flags are what the step produced. */
IRLOSC_API int irlosc_rollout_from_q_logged(irlosc_ctx* ctx, int32_t slot, int32_t B, int32_t ticks, const irlosc_log* log,
                                            const int32_t* robots, double* log_host, void* u_host, uint32_t* flags_any_host);

/* ---- episodes: per-robot resets on the GPU and an early exit of the rollout (csrc/osc_episode.hpp) -----------------------------------
 * A rollout is one episode per robot per call unless the slot has EPISODES: then a robot whose episode has ended starts over on the
 * device while its neighbours go on, and a call can end as soon as every robot is through.  One more small kernel per tick, behind the
 * plant (which wrote the coordinates a reset replaces): the last launch of the tick.  Per covered robot the device keeps
 *     count        episodes ended so far
 *     age          ticks the running episode has been run (only ticks that run the robot count: a rollout over fewer robots does not
 *                  age those it leaves out -- the list's own "first tick that runs it" rule)
 *     start_tick   the episodes' tick on which the running episode first ran (-1: it has not run yet)
 *     a ring of the last `records` ended episodes: start_tick, length (= age), outcome, start index | variant index << 16
 * and judges it on every tick that runs it.  The episode ENDS on that tick when
 *     FINISHED, with end_on_finish:  a LIST: the robot's finished_tick >= 0;  PATHS: every listed device with loop == 0 has index == W_d,
 *                                    and there is such a device;  no program, a policy: never;  and, whatever the program, on a
 *                                    slot whose reward has a goal: the robot's goal_step >= 0 (IRLOSC_EPISODE_GOAL, below)
 *     TIMEOUT, with max_ticks > 0:   age == max_ticks.  A robot that finishes on the tick of its timeout is FINISHED.
 * Then its record is written and count += 1, and with max_episodes == 0 || count < max_episodes the robot is RESET, else PARKED: never
 * judged again, it carries on exactly as a finished robot does without episodes.  A reset leaves the robot as the setters' init launches
 * would: coordinates (walk layout, row-major qpos and qvel) = start state count mod S; its whole target row = the snapshot taken by
 * irlosc_set_episodes (PATHS: waypoint 0 of every listed device on top); a list's state as irlosc_set_action_list leaves it, word 9 of
 * the active device in the slot's gain copy taken again from the context's gains and, with V > 0 pose variants, the robot's lines of the
 * list's pose table rewritten with variant count mod V; the paths' state (0, 0, -1); walls: force, max_depth, contact_ticks 0,
 * first_tick -1 (the SENSE launch of the next tick subtracts +0.0: the feed's wrench keeps its bits); joint rows: tau, max_violation,
 * active_ticks 0 and ctrl 0 (an ACTION drive lets go).  The next tick is the first tick of a fresh rollout for that robot.  Tick-valued
 * state (finished_tick, last_tick, first_tick) keeps counting its owner's ticks: subtract the episode's start_tick.
 * "The first tick of a fresh rollout" is meant bit for bit WITHIN ONE FORM OF THE EIGEN PASS: which form a step runs follows from how
 * many robots of the fleet are flagged on that tick (IRLOSC_LANE_EIG_MIN), and in a rollout with episodes that number differs from any
 * fresh rollout's.  A fleet that stays on one side of the threshold (or a process with the form pinned) repeats its fresh rollouts'
 * bits; one that crosses it repeats them to the two forms' agreement (1e-9 relative) only.
 * EARLY EXIT.  poll_every = P > 0: after the ticks P - 1, 2 P - 1, ... of a call the number of robots of the call that are not parked
 * goes to pinned host memory behind an event on the rollout's stream; before enqueuing tick m P (m >= 2) the host WAITS for the copy
 * made after tick (m - 1) P - 1 and ends the call there if it is zero.  Waiting, not polling: the ticks a call runs are a function of
 * its inputs.  With D the tick of the call on which its last robot parks (-1: all were parked before it):
 *     ticks_run = min(ticks, (max(1, ceil((D + 1) / P)) + 1) P);   ticks where no such tick exists, or with P == 0.
 * An unlogged and a logged call exit alike; a logged one drains the samples of the half it stopped in and leaves the rows of log_host
 * beyond the ticks run unwritten; u_host / flags_any_host are those of the last tick run.  Without episodes, or with poll_every == 0,
 * a rollout enqueues exactly what it enqueued before. */
#define IRLOSC_EPISODE_FINISHED 1
#define IRLOSC_EPISODE_TIMEOUT  2
#define IRLOSC_EPISODE_INSERTED 4             /* OR-ed into the outcome on a slot with mates ("action objects", below): every mate of the
                                                 slot has mated_tick >= 0 on the tick the episode ends -- 5 or 6 in place of 1 or 2 */
#define IRLOSC_EPISODE_GOAL     8             /* OR-ed into the outcome on a slot whose reward has a goal ("a reward per tick", above): the
                                                 robot's goal_step >= 0 on the tick the episode ends.  With end_on_finish such an episode is
                                                 FINISHED on that tick, whatever the program -- a policy's and no program's included */
#define IRLOSC_MAX_EPISODE_RECORDS 16
#define IRLOSC_MAX_EPISODE_STARTS  4096       /* start states and pose variants, each */
typedef struct irlosc_episodes {
    int32_t max_ticks;          /* >= 0: 0 = no timeout */
    int32_t end_on_finish;      /* 0 / 1 */
    int32_t max_episodes;       /* >= 0: 0 = no limit; else a robot parks when it has ended this many */
    int32_t n_starts;           /* S in [1, IRLOSC_MAX_EPISODE_STARTS] */
    int32_t starts_per_robot;   /* 0: one set of S start states for the fleet, 1: a set per robot */
    int32_t n_variants;         /* V in [0, IRLOSC_MAX_EPISODE_STARTS]: pose variants of the slot's action list (0: its table stays) */
    int32_t records;            /* ring length in [1, IRLOSC_MAX_EPISODE_RECORDS] */
    int32_t poll_every;         /* P >= 0: 0 = never exit early */
    int32_t reserved;           /* 0 */
} irlosc_episodes;
/* Gives slot `slot`'s B robots their episodes: qpos0, qvel0 [starts_per_robot ? B : 1][S][n] double, poses [V][B][A][7] double (A: the
 * list's n_actions; rows of GRIP actions are not read; NULL with V == 0).  Every argument is checked before anything is touched
 * (IRLOSC_ERR_ARG: a field outside its range above, reserved != 0, B < 1, qpos0 / qvel0 NULL or poses NULL with V > 0, a start state or
 * the pose of a WP that is not finite).  IRLOSC_ERR_STATE, with the reason, and the episodes in force stay: no model; targets, or the
 * slot's program, walls or joint rows covering fewer than B robots; a context whose n is not the rollout's; a teleoperation stream or
 * pushes on the slot (and those two setters are refused on a slot with episodes); V > 0 without an action list, or with one whose pose
 * table is shared by the fleet (nb == 1 for more than one robot).  On success: count 0, age 0, start_tick -1, tick base 0, the ring
 * zero, the snapshot of the slot's targets taken, start state 0 written into the coordinates of the B robots (as irlosc_set_waypoints
 * writes waypoint 0 into the targets: the slot then has coordinates for B robots) and variant 0 into the list's pose table.  The
 * program's own state is NOT reset: set the program, then its episodes.  desc == NULL ends the episodes; what else ends them: "one
 * writer of the targets" above.  Buffers are allocated by the first use; IRLOSC_ERR_HIP leaves the slot without episodes.  Synchronous. */
IRLOSC_API int irlosc_set_episodes(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_episodes* desc, const double* qpos0,
                                   const double* qvel0, const double* poses);
/* count, age, start_tick: int32 [B]; running: one int32, the robots of the first B that are not parked; records [B][records][4] int32
 * (start_tick, length, outcome, start index | variant index << 16), entry e of a robot being its episode e' = the largest e' < count
 * with e' mod records == e (entries >= count: zero); ticks_run: one int32, the ticks the slot's last rollout call ran.  Any may be NULL.
 * IRLOSC_ERR_STATE on a slot without episodes, or with episodes for fewer than B robots -- but B == 0 answers ticks_run on any slot.
 * Synchronous. */
IRLOSC_API int irlosc_download_episode_state(irlosc_ctx* ctx, int32_t slot, int32_t B, int32_t* count, int32_t* age, int32_t* start_tick,
                                             int32_t* running, int32_t* records, int32_t* ticks_run);

/* ---- action objects: kinematic bodies the gripper carries, and an insertion outcome (csrc/osc_object.hpp) --------------------------
 * The insertion demo grips the male part, carries it to the female part and releases it there; in the reference a WP reads an object's
 * pose from the simulator when it is entered (insertion_task.py:226-262).  OBJECTS give a slot's rollouts that much of it, and no more:
 * an object rides rigidly on an EE once that arm's fingers have closed near it, stays where it is let go, a WP of the slot's action
 * list can aim at its live pose, and a plug released inside its socket's tolerances is recorded.  With LOADS (irlosc_set_object_loads,
 * below) a held object also has a weight, which the plant and the F/T feed see.  What this is NOT: no inertial force (the weight is
 * quasi-static: m g, never m a), no fall (a released object hangs where it was let go, and a free one weighs on nothing), no collision, no
 * slipping, and the fingers' forces are not in the feed.
 * One more small kernel per tick, behind the walk (and the feed's SENSE launches) and directly in front of the action kernel, so a WP
 * entered on tick t sees the objects of tick t.  Float64 whatever the context's dtype, only + - x, comparisons and the one correctly
 * rounded division of quat2mat (2 / |q|^2), every operation rounded on its own: irl_control_amd/objects.py::object_step repeats the bits.
 * Per robot the device keeps, per object: pose[7] (x y z qw qx qy qz), holder (-1 = free, else the gripper), rel[7] (its pose in the
 * holder's EE frame), grasp_tick, release_tick (the objects' ticks, -1: never); per gripper was_closed; per mate mated_tick (-1: not yet).
 *   GRIPPER g: device dev[g] (targets order), knuckle hinge joint[g], sign[g] in {+1, -1}, q_close[g], q_open[g] with
 *              sign q_open < sign q_close, grip_xyz[g] a point in the EE frame.  With q the knuckle coordinate at the start of the tick:
 *              closed = sign q >= sign q_close, open = sign q <= sign q_open, a NaN is neither.
 *   OBJECT o:  radius[o] >= 0.
 *   MATE m:    plug[m] != socket[m], seat_xyz[m] / seat_quat[m] in the socket's frame, tol_xyz[m] > 0, min_abs_dot[m] in [0, 1].
 * Per tick t and covered robot, T_ee = (p_ee, q_ee) the EE pose of a gripper's device, R() = quat2mat:
 *   0. an EE pose word of a gripper's device that is not finite: objects, grippers and mates of the robot stay as they are
 *   1. held objects, ascending o:  holder open -> holder = -1, release_tick = t, the pose stays;
 *                                  else xyz = p_ee + R(q_ee) rel_xyz, quat = q_ee (x) rel_quat
 *   2. free objects not released on this tick, ascending o, grippers ascending g: g closed, was_closed[g] == 0 (the rising edge: a hand
 *      that travels closed picks nothing up), g holds nothing, |p_ee + R(q_ee) grip_xyz - p_obj|^2 <= radius^2
 *      -> holder = g, rel_xyz = R(q_ee)^T (p_obj - p_ee), rel_quat = conj(q_ee) (x) q_obj, grasp_tick = t
 *   3. was_closed[g] = closed(g)
 *   4. mates, ascending m, with mated_tick < 0 and the plug free: target xyz = p_sock + R(q_sock) seat_xyz, quat = q_sock (x) seat_quat;
 *      |p_plug - target|^2 <= tol_xyz^2 and |q_plug . q_target| >= min_abs_dot -> mated_tick = t
 * Episodes (above) reset a robot's objects with the rest of it: free, pose = start poses count mod V, ticks -1, was_closed 0; and on a
 * slot with mates the record's outcome carries IRLOSC_EPISODE_INSERTED.  Order of calls: program, objects, loads, refs, then episodes.
 * A slot without objects launches exactly the kernels it launched before. */
#define IRLOSC_MAX_OBJECTS  4
#define IRLOSC_MAX_GRIPPERS 2
#define IRLOSC_MAX_MATES    2
typedef struct irlosc_objects {
    int32_t n_objects;                               /* in [1, IRLOSC_MAX_OBJECTS] */
    int32_t n_grippers;                              /* in [1, IRLOSC_MAX_GRIPPERS] */
    int32_t n_mates;                                 /* in [0, IRLOSC_MAX_MATES] */
    int32_t n_variants;                              /* V in [1, IRLOSC_MAX_EPISODE_STARTS]: sets of start poses (episodes cycle them) */
    int32_t dev[IRLOSC_MAX_GRIPPERS];                /* device in [0, ndev) */
    int32_t joint[IRLOSC_MAX_GRIPPERS];              /* knuckle hinge in [0, n) */
    int32_t sign[IRLOSC_MAX_GRIPPERS];               /* +1 / -1 */
    int32_t plug[IRLOSC_MAX_MATES];                  /* object in [0, n_objects) */
    int32_t socket[IRLOSC_MAX_MATES];                /* ... another one */
    double q_close[IRLOSC_MAX_GRIPPERS];
    double q_open[IRLOSC_MAX_GRIPPERS];
    double grip_xyz[IRLOSC_MAX_GRIPPERS][3];
    double radius[IRLOSC_MAX_OBJECTS];
    double seat_xyz[IRLOSC_MAX_MATES][3];
    double seat_quat[IRLOSC_MAX_MATES][4];
    double tol_xyz[IRLOSC_MAX_MATES];
    double min_abs_dot[IRLOSC_MAX_MATES];
} irlosc_objects;
/* Gives slot `slot`'s B robots their action objects: pose0 [V][B][n_objects][7] double.  Every argument is checked before anything is
 * touched (IRLOSC_ERR_ARG: a count outside its range above, B < 1, a device, hinge or object index out of range, plug == socket, sign
 * not +-1, pose0 NULL, a value that is not finite, sign q_open >= sign q_close, radius < 0, tol_xyz <= 0, min_abs_dot outside [0, 1];
 * the objects in force stay, whole).  IRLOSC_ERR_STATE: before irlosc_set_model, or before the slot has coordinates for B robots
 * (irlosc_upload_q).  desc == NULL clears.  On success the state is that of variant 0: every object free at its start pose, ticks -1,
 * was_closed 0, the objects' tick base 0; the list's refs (below) end.  A rollout over more robots than the objects cover answers
 * IRLOSC_ERR_STATE, and so does irlosc_set_episodes for more robots than they cover.  The model's change ends them.  Buffers are
 * allocated by the first use; IRLOSC_ERR_HIP leaves the slot without objects.  Synchronous. */
IRLOSC_API int irlosc_set_objects(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_objects* desc, const double* pose0);
/* The objects' per-robot state of the slot's first B robots: pose[B][n_objects][7], rel[B][n_objects][7] (double), holder, grasp_tick,
 * release_tick [B][n_objects], mated_tick[B][n_mates] (int32); any may be NULL.  IRLOSC_ERR_STATE: the slot has no objects, or they
 * cover fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_object_state(irlosc_ctx* ctx, int32_t slot, int32_t B, double* pose, int32_t* holder, double* rel,
                                            int32_t* grasp_tick, int32_t* release_tick, int32_t* mated_tick);
/* The slot's objects get a WEIGHT (csrc/osc_object_load.hpp): per object a mass and a centre of mass in the object's frame, and a gravity
 * vector.  A gripper that holds an object feels the weight as a wrench on its device's EE body, at the body's frame origin, the way a wall's
 * force is felt (irlosc_set_walls): computed on the device per robot and tick, added to the bias in front of the plant -- behind the pushes
 * and the walls, in front of the joint rows -- remembered for one tick and taken off the feed's wrench on the next (slots with a feed,
 * devices with a sensor), all six words.  Per tick and gripper g, ascending, with o the lowest object whose holder is g after this tick's
 * object kernel:
 *     no such object, or mass[o] == 0:   W_g = 0
 *     else   c = R(q_obj) com,  p_c = p_obj + c,  r = p_c - p_ee,  F = mass gravity,  T = r x F,  W_g = (F, T)
 *     a word of W_g that is not finite:  W_g = 0 on this tick, and the tick is not counted
 *     unless W_g is all zero:            bias_i = fma(-J[5][i], W5, ... fma(-J[0][i], W0, bias_i)) on every hinge above the EE body -- the
 *                                        pushes' chain -- and carry_ticks[g] += 1
 * Float64 whatever the context's dtype, every operation rounded on its own: irl_control_amd/object_loads.py::load_wrench repeats the bits.
 * QUASI-STATIC: the object's inertial force m a is not modelled; nothing falls, collides or slips, and the fingers' forces are not in the
 * feed.  The existing wrench channel of the log carries the sensed weight; there is no channel of its own.
 * table: [n_objects][4] (per_robot == 0: shared by the fleet) or [B][n_objects][4]; row of object o: mass (>= 0), com_x com_y com_z in the
 * object's frame.  Every argument is checked before anything is touched (IRLOSC_ERR_ARG: B < 1, table NULL, a value that is not finite,
 * mass < 0, per_robot outside {0, 1}, reserved != 0; the loads in force stay, whole).  IRLOSC_ERR_STATE: the slot has no objects, or they
 * cover fewer than B robots.  desc == NULL clears the loads and leaves the objects' state untouched.  irlosc_set_objects, set or clear,
 * ends the loads, and so does the model's change.  On success the per-robot state is zero -- load 0, carry_ticks 0 -- and the loads' tick
 * base is 0.  A rollout over more robots than the loads cover answers IRLOSC_ERR_STATE.  Episodes reset a robot's load words and
 * carry_ticks to zero.  Buffers are allocated by the first use; IRLOSC_ERR_HIP leaves the slot without loads.  A slot without loads
 * launches exactly the kernels it launched before.  Synchronous. */
typedef struct irlosc_object_loads {
    int32_t per_robot;                               /* 0: table [n_objects][4] shared by the fleet; 1: [B][n_objects][4] */
    int32_t reserved;                                /* 0 */
    double gravity[3];                               /* world frame, e.g. 0 0 -9.81 */
} irlosc_object_loads;
IRLOSC_API int irlosc_set_object_loads(irlosc_ctx* ctx, int32_t slot, int32_t B, const irlosc_object_loads* desc, const double* table);
/* The loads' per-robot state of the slot's first B robots: load[B][n_grippers][6] (double: the wrench the last tick applied per gripper,
 * fx fy fz tx ty tz, world frame), carry_ticks[B][n_grippers] (int32: ticks on which a weight was applied); either may be NULL.
 * IRLOSC_ERR_STATE: the slot has no loads, or they cover fewer than B robots.  Synchronous. */
IRLOSC_API int irlosc_download_object_load_state(irlosc_ctx* ctx, int32_t slot, int32_t B, double* load, int32_t* carry_ticks);
/* The slot's action list aims at its objects.  For a WP action a with xyz_obj[a] >= 0 the xyz words of the list's pose a are an OFFSET:
 * on entry, target xyz = the object's xyz + offset, one add per word (the reference's obj_pos + offset); xyz_from_start wins.  With
 * quat_obj[a] >= 0 the quaternion words are the grip rotation: target quat = q_obj (x) q_grip, the Hamilton product with its terms left
 * to right, no normalisation, no sign change (the reference reaches the same rotation through mat2euler -> set_abg: equal up to the
 * quaternion's sign, which calc_error does not see).  Targets are read at ENTRY only: a held object does not drag a target along.
 * Entries of GRIP actions and beyond n_actions are not read.  IRLOSC_ERR_ARG: an entry of a WP that is neither -1 nor an object index.
 * IRLOSC_ERR_STATE: the slot has no action list, no objects, or objects that cover fewer robots than the list; the refs in force stay.
 * refs == NULL clears.  irlosc_set_action_list and irlosc_set_objects end the refs (set them last).  Pose variants of episodes
 * rewrite offsets and grip rotations like any other pose word.  Without refs the list's kernel computes what it computed before. */
typedef struct irlosc_action_refs {
    int32_t xyz_obj[IRLOSC_MAX_ACTIONS];
    int32_t quat_obj[IRLOSC_MAX_ACTIONS];
} irlosc_action_refs;
IRLOSC_API int irlosc_set_action_refs(irlosc_ctx* ctx, int32_t slot, const irlosc_action_refs* refs);

/* ---- multi-GPU: the final throughput reduction -----------------------------------------------
 * Instances are independent (osc.py:120-210 touches one robot), so a node runs one process per GPU on its own shard
 * and NOTHING is exchanged per tick.  RCCL (over xGMI) is used once per benchmark: sum of the steps done, max of the
 * elapsed time, and an all-gather of per-rank output checksums.  librccl is loaded on first use (dlopen), so a
 * single-GPU deployment does not depend on it.  The 128-byte unique id is made by rank 0 (irlosc_comm_unique_id) and
 * handed to the other ranks by the host program (irl_control_amd/sharding.py: a file next to MASTER_PORT). */
typedef struct irlosc_comm irlosc_comm;
#define IRLOSC_COMM_ID_BYTES 128
IRLOSC_API int irlosc_comm_unique_id(uint8_t id_out[IRLOSC_COMM_ID_BYTES]);
IRLOSC_API int irlosc_comm_create(int32_t hip_device, int32_t rank, int32_t world, const uint8_t id[IRLOSC_COMM_ID_BYTES],
                       irlosc_comm** out);
IRLOSC_API void irlosc_comm_destroy(irlosc_comm* comm);
IRLOSC_API const char* irlosc_comm_last_error(const irlosc_comm* comm);   /* comm may be NULL: last create()/unique_id() error */
/* In place: *steps_sum <- sum over ranks, *elapsed_max <- max over ranks (two ncclAllReduce on the comm's stream,
 * then a stream sync).  Doubles as the barrier of the benchmark bracket. */
IRLOSC_API int irlosc_bench_allreduce(irlosc_comm* comm, double* steps_sum, double* elapsed_max);
/* all[r] <- rank r's `mine` (ncclAllGather): per-shard output checksums, to show that sharding changes no bit. */
IRLOSC_API int irlosc_comm_allgather_u64(irlosc_comm* comm, uint64_t mine, uint64_t* all);

#ifdef __cplusplus
}
#endif
#endif /* IRLOSC_H */
