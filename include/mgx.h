/* mgx.h — C ABI of the MI355X-native GBP message-passing engine.
 *
 * Drop-in boundary for the factor-graph inner loop of AU-Master-Thesis/magics.
 * The reference has no FFI seam; the seam is the public Rust API of `FactorGraph`
 * (crates/magics/src/factorgraph/factorgraph.rs:76) as driven by
 * crates/magics/src/planner/robot.rs.  Because GPU execution is batched over all
 * robots, the ABI is world-level: one `mgx_world` owns every robot's factor graph
 * (device resident, SoA) and each entry point names the reference call it replaces.
 *
 * Conventions: plain C, caller owns every buffer it passes, the library owns all
 * device memory.  Every call returns an `int` status (MGX_OK == 0, negative =
 * error, never aborts).  A world is thread-compatible (external synchronisation).
 * All floating point is f64 (crates/gbp_linalg/src/lib.rs:31), DOFS = 4
 * (crates/magics/src/factorgraph/mod.rs:21).  Matrices are row-major.
 *
 * There is NO CPU fallback: every compute entry point fails with
 * MGX_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef MGX_H
#define MGX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_DOFS 4

/* status codes */
#define MGX_OK 0
#define MGX_ERR_INVALID (-1)   /* bad argument (null pointer, index out of range, K < 2 ...) */
#define MGX_ERR_NO_DEVICE (-2) /* no usable HIP device / HIP runtime error at init */
#define MGX_ERR_HIP (-3)       /* HIP runtime call failed (see mgx_last_error) */
#define MGX_ERR_STATE (-4)     /* call not valid in the current state */
#define MGX_ERR_NOMEM (-5)

/* factor kinds, bit positions of mgx_params.enable_mask
 * (gbp_config FactorsEnabledSection, crates/gbp_config/src/lib.rs:454-494) */
#define MGX_FACTOR_DYNAMIC 1u
#define MGX_FACTOR_INTERROBOT 2u
#define MGX_FACTOR_OBSTACLE 4u
#define MGX_FACTOR_TRACKING 8u

/* one schedule step, bits of the uint8 passed to mgx_iterate
 * (gbp_schedule::GbpScheduleAtIteration, crates/gbp_schedule/src/schedules/mod.rs:59-63) */
#define MGX_STEP_INTERNAL 1u
#define MGX_STEP_EXTERNAL 2u

/* schedule kinds (crates/gbp_schedule/src/schedules/ *.rs) */
#define MGX_SCHEDULE_CENTERED 0
#define MGX_SCHEDULE_SOON_AS_POSSIBLE 1
#define MGX_SCHEDULE_LATE_AS_POSSIBLE 2
#define MGX_SCHEDULE_INTERLEAVE_EVENLY 3
#define MGX_SCHEDULE_HALF_BEGINNING_HALF_END 4

typedef struct mgx_world mgx_world;

/* World-wide GBP parameters: the values `RobotBundle::new` and
 * `create_interrobot_factors` read from `Config` (robot.rs:1134-1356,1441-1586).
 * Sigmas are the f32 config values already widened to f64 (`Float::from(f32)`). */
typedef struct mgx_params {
    double sigma_dynamics;           /* config.gbp.sigma_factor_dynamics   */
    double sigma_interrobot;         /* config.gbp.sigma_factor_interrobot */
    double sigma_obstacle;           /* config.gbp.sigma_factor_obstacle   */
    double sigma_tracking;           /* config.gbp.sigma_factor_tracking   */
    double safety_multiplier;        /* config.robot.inter_robot_safety_distance_multiplier */
    double tracking_switch_padding;  /* config.gbp.tracking.switch_padding (f32 widened)      */
    double tracking_attraction_distance; /* config.gbp.tracking.attraction_distance          */
    uint32_t enable_mask;            /* MGX_FACTOR_* bits: config.gbp.factors_enabled        */
    uint32_t reserved;
} mgx_params;

/* One robot = one reference `FactorGraph` built by `RobotBundle::new`
 * (robot.rs:1134-1356): K variables, K-1 dynamic factors, K-2 obstacle factors and
 * K-2 tracking factors (on variables 1..K-2). */
typedef struct mgx_robot_desc {
    uint32_t K;               /* number of variables (>= 2)                                  */
    uint32_t n_path;          /* tracking polyline points (0 = none)                         */
    const double *mean0;      /* [K][4] initial variable means (robot.rs:1187-1218)          */
    const double *prior_diag; /* [K] diagonal of the prior precision; non-finite => 0
                                 (variable.rs:146-148); the reference uses 1e30 / +inf      */
    const double *dt;         /* [K-1] dynamic-factor delta_t (robot.rs:1232,1240)           */
    const float *path_xy;     /* [n_path][2] f32 waypoints for the tracking factors or NULL  */
    double radius;            /* robot radius; d_safe = safety_multiplier * radius           */
    uint64_t order_key;       /* total order of graphs = Bevy Entity order (id.rs:19-117);
                                 must be unique per world (across ranks when sharded, and across
                                 groups); it is only ever COMPARED between robots of one group  */
    uint32_t ghost;           /* 1 = halo copy of a robot owned by another rank: only its
                                 variable->factor snapshots exist, filled by mgx_halo_unpack */
    uint32_t group;           /* the independent run this robot belongs to (ROBOT GROUPS below),
                                 < MGX_GROUPS_MAX; 0 = the one run of an ungrouped world (the word
                                 was reserved and 0)                                           */
} mgx_robot_desc;

/* ---- ROBOT GROUPS: many independent runs in one world ---------------------------------------------------------------
 * A robot's graph couples to other robots only through inter-robot factors, so robots that are never connected are independent
 * runs already: M runs (the seeds and parameters of an experiment, a few dozen robots each) can share one world, one launch per
 * schedule and one synchronisation per tick, and every run stays bit-identical to the same run in a world of its own.  A world is
 * GROUPED once any robot has been added with a non-zero `group`; a world whose robots are all in group 0 takes exactly the code
 * paths it took before groups existed (the same search kernels, the same collision kernels, the same events).  In a grouped world:
 *   * robots of different groups are never in comms range of one another — in mgx_neighbours, mgx_update_topology, both halves of
 *     the mission tick, the search mgx_mission_tick_end enqueues for the coming tick, and the compacted queries over the alive
 *     robots.  Within a group the predicate is unchanged (a NaN distance is in range; radius 0, negative, NaN as before).  The
 *     search is ONE one-pass kernel whatever the method, MGX_SEARCH_ROWS_GROUPS: a workgroup serves sixteen robots of one group and
 *     stages and tests that group's positions only, so a search costs the sum of the squared group sizes, not the square of the
 *     world's size.  A group of more than 4096 robots in one query is refused (MGX_ERR_INVALID);
 *   * the comms radius is per group with mgx_neighbours_groups, mgx_update_topology_groups_radii and
 *     mgx_mission_tick_begin_groups_radii: radii [n_groups], by group id; a pair is tested against the radius of ITS group, each
 *     radius meaning what the scalar means (NaN: everybody of the group in range; zero, negative: as before).  The kernel and the
 *     number of launches are the same: a workgroup reads its group's threshold from a table the host keeps beside the query's
 *     group lists and uploads again only when a radius changes or robots join or leave the query — not per search.  The search
 *     mgx_mission_tick_end enqueues for the coming tick uses the radii of the last _begin; the next _begin takes those rows only if
 *     every radius is still the one they were searched with, and searches again otherwise.  radii NULL, a robot whose group is
 *     not below n_groups, n_groups outside 1 .. MGX_GROUPS_MAX: MGX_ERR_INVALID, nothing changes.  On an ungrouped world
 *     (n_groups 1) the call is the scalar call with radii[0], on the kernels that one runs.  The calls with ONE radius
 *     (mgx_update_topology_groups, mgx_mission_tick_begin_groups) are these with all radii equal;
 *   * robots of different groups never collide (mgx_collisions_update, and the pass at every tick's end).  Within a group the
 *     predicate, the Free / Colliding state machine, the event order, the per-robot counts and the overflow rules are unchanged;
 *   * the RobotNumberGenerator, whose numbers enter the arithmetic of the inter-robot factors, is per group with
 *     mgx_update_topology_groups / mgx_mission_tick_begin_groups: a connection is numbered from the generator of its creating
 *     robot's group.  Within a group the creation order (robot id ascending, row order) and the deletion quirk (the largest
 *     out-of-range key per robot) are the existing ones.  The single-generator calls keep working on a grouped world: one shared
 *     generator, grouped search.  mgx_mission_run has ONE generator and ONE stream of comms draws: per-group many-tick runs are
 *     not part of it;
 *   * the GBP iteration schedule is per group with mgx_iterate_groups and mgx_mission_tick_end_groups: group g runs
 *     steps[step_first[g] .. step_first[g + 1]), step_first [n_groups + 1] ascending from 0.  Every robot of group g runs
 *     mgx_iterate with group g's steps, bit for bit what the same robots compute in a world of their own: beliefs, means,
 *     covariances, factor -> variable messages, inter-robot messages, iteration_count.factor, the tracking factors' records and
 *     mgx_message_counts.  A group whose range is empty sits the call out.
 *     EQUAL schedules — all groups that hold live robots have byte-equal steps, an ungrouped world (n_groups 1) among them — are
 *     the plain call with those steps, through the same door: resident launch, lingering, post merging, batches, mgx_last_sweep
 *     and mgx_resident_stats as after mgx_iterate / mgx_mission_tick_end.
 *     MIXED schedules run launch by launch in the segments form: each group's steps are flattened to its own [external] internal*
 *     segments and launch k carries segment k of every group — a robot's workgroup reads its group's segment from a table in place
 *     of the kernel's scalars, and a workgroup whose group has no segment k (fewer segments, an empty range) sits the launch out:
 *     it stages nothing and only carries its snapshot records over where the launch writes snapshots (mgx_group_schedule_stats
 *     counts them).  mgx_last_launch_count is the largest segment count over the groups, mgx_last_sweep reports
 *     MGX_SWEEP_FORM_SEGMENTS.  Like every other call, a mixed call first ends a lingering launch and submits recorded schedules,
 *     an open batch's included.  The prior updates of a mixed mgx_mission_tick_end_groups go as the kernel of their own — what
 *     mgx_update_priors followed by mgx_iterate does: the same result (mgx_tick below).  The observer passes at the tick's end
 *     are unchanged, and the call pairs with any of the _begin forms.
 *     MGX_ERR_INVALID, nothing changes: steps NULL with steps to read, step_first NULL, n_groups outside 1 .. MGX_GROUPS_MAX, a
 *     step byte with a bit that is no MGX_STEP_* (its index is named), step_first not ascending from 0, a live robot whose group
 *     is not below n_groups.  The arguments are checked before the world is touched; a NULL world is reported last.
 *     MGX_ERR_STATE, nothing changes: a mixed schedule on a sharded world (ghosts have no group, and every robot there is in group
 *     0: a call whose groups do not ALL have byte-equal steps is refused, whichever of them hold robots), and on a world that has
 *     ever switched a factor kind with mgx_set_enabled (the thaw kernels in front of a sweep are world-wide).
 *     The open end: a mixed call is never recorded, posted or run resident;
 *   * the enabled factor kinds (gbp.factors-enabled) are per group with mgx_set_group_enabled: every factor of a robot of group g
 *     is enabled iff its kind's bit is set in group g's mask.  A group that was never given a mask has the world's
 *     (mgx_params.enable_mask, or what mgx_set_enabled made of it), and a mask equal to the world's is no mask at all: the group
 *     follows the world as if the call had not been made.  The INTERNAL kinds may differ from the world's (MGX_FACTOR_DYNAMIC,
 *     _OBSTACLE, _TRACKING: bits 1, 4, 8).  The inter-robot bit must equal the world's — it decides residency, keyless factors and
 *     the inter-robot freeze world-wide — MGX_ERR_INVALID otherwise.
 *     A group's kinds are fixed for the life of the group: the call is accepted only while no robot of that group has ever been
 *     added (group 0 counts like any other), MGX_ERR_STATE afterwards.  So a factor of a switched-off kind is off FROM ITS
 *     CREATION and never switched on: it receives nothing, not even the empty message of add_internal_edge
 *     (factorgraph.rs:304-330, mgx_message_counts); it sends nothing; its variable does not deliver to it
 *     (factorgraph.rs:695,781) — what the same robots do in a world of their own created with that mask in mgx_params, bit for
 *     bit, as everything else of a group.
 *     A world is MASKED while some group's mask differs from the world's.  A masked world runs EVERY schedule launch by launch,
 *     as mixed schedules run: mgx_iterate, mgx_iterate_groups, mgx_tick, mgx_mission_tick_end(_groups), open batches and the
 *     world-wide mgx_sweep / mgx_*_iteration calls become launches in which every workgroup reads its group's kinds from a table
 *     beside the group's segment record (equal schedules: every group the same segments); a per-robot fine-grained call hands
 *     the kinds of that robot's group to its launch.  Prior updates go as the kernel of their own, as in mixed calls.  Never
 *     recorded, posted or resident: mgx_last_sweep reports MGX_SWEEP_FORM_SEGMENTS.  mgx_group_enabled_stats counts the schedules
 *     (and world-wide sweeps) that ran this way BECAUSE of the masks; mixed calls keep counting in mgx_group_schedule_stats.
 *     mgx_set_group_resident(w, 1) changes that for the world's EQUAL schedules (off by default): mgx_iterate, mgx_iterate_groups
 *     and mgx_mission_tick_end_groups with equal schedules, mgx_tick, mgx_mission_tick_end and batches then run as on an unmasked
 *     world — one resident launch of the masked form of the kernel (MGX_SWEEP_F_GROUP_KINDS: each workgroup reads its group's
 *     kinds once, from the table that is uploaded in front of the launch and never written while one lingers), lingering, posts,
 *     post merging, the residency census, prior updates riding in the launch or the post.  Mixed schedules and the world-wide
 *     fine-grained sweeps stay group plans.  A schedule that cannot run resident (no connection yet, mgx_set_resident_launches 0,
 *     a launch the census declined, the rest of a plan after a back-off, a post taken back) sends its prior updates as the
 *     kernel of their own and runs as ONE group plan: mgx_group_enabled_stats counts it, and so does `fallbacks` of
 *     mgx_group_resident_stats.  Results are the same bit for bit either way.  On an unmasked world the switch does nothing.
 *     An unmasked world, grouped or not, takes exactly the code paths it took before the call existed.
 *     MGX_ERR_STATE, nothing changes: a world that has switched a factor kind at run time (mgx_set_enabled with robots: freeze
 *     and thaw are world-wide), a world with ghosts or an engine-side exchange.  On a masked world mgx_set_enabled with a mask
 *     other than the world's and mgx_mission_run (one generator, one schedule: one group's) are MGX_ERR_STATE.
 *     The arguments are checked first and need no device: unknown kind bits, then group >= MGX_GROUPS_MAX (both
 *     MGX_ERR_INVALID), a NULL world or out-pointer last;
 *   * the four factor sigmas (gbp.sigma-factor-{dynamics, interrobot, obstacle, tracking}) are per group with
 *     mgx_set_group_sigmas, under the rules of mgx_set_group_enabled: before the group's first robot (MGX_ERR_STATE afterwards), a
 *     group never given sigmas has the world's (mgx_params.sigma_*), and a set equal to the world's is none at all.  Every robot
 *     of group g then runs under g's sigmas — its dynamic factors' potentials are formed with g's sigma_dynamics when it is added
 *     (spawned in place included), its obstacle, tracking and inter-robot factors (which only ever join robots of one group) are
 *     evaluated with g's 1 / sigma^2, the double a world created with those mgx_params holds — bit for bit what the same robots
 *     do in a world of their own created with those sigmas.  A group may have both a mask and sigmas.
 *     A world in which some group's sigmas differ from the world's is run exactly as a MASKED world is (above): group plans
 *     launch by launch, each workgroup reading its group's three 1 / sigma^2 from a second table beside the kinds'; a
 *     per-robot fine-grained call hands its launch that robot's group's; with mgx_set_group_resident(w, 1) resident launches
 *     and posts of the masked form, which reads the table once per workgroup.  mgx_group_enabled_stats and
 *     mgx_group_resident_stats count its plans and launches as a masked world's; mgx_set_enabled with another mask and
 *     mgx_mission_run are MGX_ERR_STATE there (the freeze and thaw kernels evaluate factors with the world's sigmas).
 *     MGX_ERR_INVALID: a NULL struct, then a value that is not finite and > 0, then group >= MGX_GROUPS_MAX — checked before the
 *     world is looked at, a NULL world last.  MGX_ERR_STATE, nothing changes: a world that has switched a factor kind at run
 *     time, a world with ghosts or an engine-side exchange.  Not per group: sigmas changed once the group has robots,
 *     tracking.switch-padding and attraction-distance, the safety multiplier.
 * Everything else is per robot and does not look at the group: prior updates, missions, trackers, run metrics, environment
 * collisions, goal areas, the planner, the message counters.
 * Ghosts have no group: mgx_robot_add of a ghost with a non-zero group is MGX_ERR_INVALID; a ghost added to a grouped world, a
 * grouped robot added to a world with ghosts, and mgx_robot_release on a grouped world are MGX_ERR_STATE.  group >= MGX_GROUPS_MAX
 * is MGX_ERR_INVALID. */
#define MGX_GROUPS_MAX 4096u

/* ---- lifecycle ------------------------------------------------------------------- */
int mgx_world_create(const mgx_params *params, mgx_world **out);
int mgx_world_destroy(mgx_world *w);
/* text of the last error on this thread (never NULL) */
const char *mgx_last_error(void);
/* HIP stream every kernel / copy of this world is enqueued on (NULL = default stream) */
int mgx_set_stream(mgx_world *w, void *hip_stream);
int mgx_synchronize(mgx_world *w);

/* Obstacle "SDF" image sampled by ObstacleFactor::measure (factor/obstacle.rs:141-188):
 * interleaved RGB u8, row-major, `world_w x world_h` world units (robot.rs:1259-1264).
 * Only the red channel is kept on the device.
 * The obstacle factors' jacobian_delta is (world_w / width + world_h / height) / 2 (obstacle.rs:98-102).  The kernels divide by
 * it through a reciprocal that the host checks against every numerator the image's 256 sample values can form; a delta for
 * which that check fails — zero, not finite, or near the ends of the f64 range: no map of any use — makes the next call that
 * commits the world (the first iterate / tick / read after a change) return MGX_ERR_INVALID, whether or not obstacle factors
 * are enabled at that moment (mgx_set_enabled can switch them on without another commit). */
int mgx_world_set_sdf(mgx_world *w, const uint8_t *rgb, uint32_t width, uint32_t height,
                      double world_w, double world_h);

/* ---- topology (FactorGraph::add_variable/add_factor/add_*_edge, robot.rs) ---------- */
/* RobotBundle::new (robot.rs:1134-1356). */
int mgx_robot_add(mgx_world *w, const mgx_robot_desc *desc, int32_t *robot_id);
/* Entity despawn (robot.rs:2172, despawn_entity_after): the robot leaves every query — never
 * iterated again, whatever is addressed to it is dropped (robot.rs:1815,1844), invisible to
 * mgx_neighbours.  Ids stay stable; its last beliefs remain readable.  The other robots drop
 * their factors towards it in the following mgx_update_topology passes (or mgx_ir_disconnect). */
int mgx_robot_remove(mgx_world *w, int32_t robot);
/* create_interrobot_factors for ONE direction (robot.rs:1500-1585): `owner` creates
 * K-1 InterRobotFactors towards `other`, variable i <-> variable i, i = 1..K-1, with
 * robot_number = first_robot_number + (i-1) (robot.rs:1527, interrobot.rs:75).
 * The reference calls this for (a,b) and (b,a) in the same system run. */
int mgx_ir_connect(mgx_world *w, int32_t owner, int32_t other, uint64_t first_robot_number);
/* delete_interrobot_factors (robot.rs:1386-1439): removes a->b and b->a factors and
 * both sides' inbox entries (factorgraph.rs:380-436). */
int mgx_ir_disconnect(mgx_world *w, int32_t a, int32_t b);

/* RadioAntenna.active (robot.rs:1593-1601) and Mission.state.idle() gates of
 * iterate_gbp_v2 (robot.rs:1794,1806,1822,1835,1851). */
/* FactorGraph::change_factor_enabled(FactorsEnabledSection) applied to every graph
 * (factorgraph.rs:1529-1539; ui/settings.rs:491-496) and to factors created from now on
 * (robot.rs:1236,1276,1326,1506 read the same config entry): MGX_FACTOR_* bits.  A disabled factor
 * keeps its last message in the variable's inbox and drops what is sent to it; switched on again it
 * resumes from the inbox it froze with (all four kinds).  On a sharded world every rank calls this with
 * the same mask right after a halo exchange (the records inter-robot factors freeze with / thaw against
 * include the ghosts' — they have to be the owners' current ones). */
int mgx_set_enabled(mgx_world *w, uint32_t kind_mask);
/* FactorGraph::update_inter_robot_safety_distance_multiplier (factorgraph.rs:892-910 -> InterRobotFactor::update_safety_distance,
 * interrobot.rs:87-89) applied to every graph and to the config entry new factors read, as the reference's only caller does
 * (ui/settings.rs:586-590): every inter-robot factor of the world gets safety_distance = multiplier * radius(owner) — frozen
 * and keyless ones included — and so does every connection created from now on and every later re-layout of the world.
 * Nothing else changes (messages, response means, epochs, counters).  Applied on the device, in place: the edge records and
 * the slot records kept there are rewritten from the robots' radii; no state is pulled, nothing is laid out again.
 * multiplier must be finite and > 0 (StrictlyPositiveFinite): MGX_ERR_INVALID otherwise, nothing changes.  On a sharded
 * world every rank calls this with the same value between the same two schedules (nothing that travels changes). */
int mgx_set_safety_multiplier(mgx_world *w, double multiplier);
int mgx_set_antenna(mgx_world *w, int32_t robot, int32_t active);
int mgx_set_idle(mgx_world *w, int32_t robot, int32_t idle);
/* The idle flag as the world holds it — set by mgx_set_idle, cleared by mgx_apply_global_paths' ACTIVATE, set by a mission
 * tick's first half for a robot that ended a leg (MISSIONS OF SEVERAL LEGS): *idle = 0 / 1.  Host state: no synchronisation. */
int mgx_get_idle(mgx_world *w, int32_t robot, int32_t *idle);

/* update_failed_comms (robot.rs:1593-1601) writes every antenna once per tick: bulk form.
 * The Bernoulli draws stay with the caller (the reference uses Bevy's GlobalEntropy<WyRand>). */
int mgx_set_antennas(mgx_world *w, uint32_t n, const int32_t *robots, const uint8_t *active);

/* ---- dynamic inter-robot topology (robot.rs:1362-1586) ----------------------------------- */
#define MGX_NEIGHBOURS_AUTO 0u  /* all-pairs kernel below 512 robots, hash grid above */
#define MGX_NEIGHBOURS_PAIRS 1u /* all-pairs kernel (what the reference does on the CPU) */
#define MGX_NEIGHBOURS_GRID 2u  /* uniform hash grid, 3x3 cells of ~radius (falls back to all
                                   pairs when radius is not positive and finite) */
/* update_robot_neighbours (robot.rs:1362-1384): `positions_xyz` = Transform::translation of
 * every robot of the world in id order (host, n x 3 f32).  Robot j is in range of i (j != i)
 * unless `radius < |p_i - p_j|` in f32 (so a NaN distance is in range).  CSR result on the
 * host: row_ptr[n+1], rows ascending in Entity order (= order_key) like the BTreeSet
 * robots_within_comms_range.  neighbours_out may be NULL to size the call (*needed). */
int mgx_neighbours(mgx_world *w, const float *positions_xyz, float radius, uint32_t method,
                   int32_t *row_ptr, int32_t *neighbours_out, uint64_t capacity,
                   uint64_t *needed);
/* One pass of update_robot_neighbours + delete_interrobot_factors + create_interrobot_factors
 * (robot.rs:86-99,1362-1586), including the reference's bookkeeping quirk: the pairs to delete
 * go through a HashMap<RobotId,RobotId> (robot.rs:1391-1404), so per robot only the
 * largest-id out-of-range peer gets its factors deleted in that pass, the rest only leave
 * robots_connected_with (and get a second set of factors if they come back in range).
 * `robot_number_next` is RobotNumberGenerator (robot.rs:122-140), advanced by one per created
 * factor.  stats (optional) = {connections created (one direction each), pairs deleted}.
 * Existing state survives: the device state is pulled to the host before the tables are
 * rebuilt, only when something changed. */
int mgx_update_topology(mgx_world *w, const float *positions_xyz, float radius, uint32_t method,
                        uint64_t *robot_number_next, uint32_t *stats);
/* The same pass with one RobotNumberGenerator per group (ROBOT GROUPS above): number_next [n_groups], in / out, none of them 0;
 * stats (optional) [n_groups][2] = {connections created by robots of the group, pairs deleted}.  Every robot's group must be
 * below n_groups, n_groups in 1 .. MGX_GROUPS_MAX (MGX_ERR_INVALID otherwise, nothing changes).  Works on an ungrouped world too
 * (n_groups >= 1, everything in group 0). */
int mgx_update_topology_groups(mgx_world *w, const float *positions_xyz, float radius, uint32_t method, uint32_t n_groups,
                               uint64_t *number_next, uint32_t *stats);
/* ... and one comms radius per group (ROBOT GROUPS above): radii [n_groups], by group id. */
int mgx_update_topology_groups_radii(mgx_world *w, const float *positions_xyz, const float *radii, uint32_t method,
                                     uint32_t n_groups, uint64_t *number_next, uint32_t *stats);
/* mgx_neighbours with one radius per group: radii [n_groups], by group id (ROBOT GROUPS above). */
int mgx_neighbours_groups(mgx_world *w, const float *positions_xyz, const float *radii, uint32_t n_groups, uint32_t method,
                          int32_t *row_ptr, int32_t *neighbours_out, uint64_t capacity, uint64_t *needed);
/* RobotConnections::robots_connected_with of one robot (robot.rs:515-531), ascending.
 * others may be NULL to query the count. */
int mgx_connections(mgx_world *w, int32_t robot, int32_t *others, uint32_t capacity, uint32_t *n);

/* ---- the hot path ------------------------------------------------------------------ */
/* iterate_gbp_v2 (robot.rs:1769-1861): runs `n` schedule steps, step i doing the
 * internal phase if steps[i] & MGX_STEP_INTERNAL and the external phase if
 * steps[i] & MGX_STEP_EXTERNAL.  Asynchronous on the world's stream.
 * While a resident launch lingers and has not yet taken the schedule posted before (LINGERING, POST MERGING below), the call
 * RECORDS its schedule instead of waiting: it reaches the device with the caller's next call on this world, whichever that is,
 * merged with its neighbours into one plan.  Results are the same bit for bit; a caller that issues schedules back to back and
 * then goes silent ends with mgx_flush, mgx_synchronize or a read (any of them submits what is recorded). */
int mgx_iterate(mgx_world *w, const uint8_t *steps, uint32_t n);
/* mgx_iterate with one schedule per robot group (ROBOT GROUPS above):
 * group g runs steps[step_first[g] .. step_first[g + 1]); step_first [n_groups + 1], ascending, step_first[0] == 0 */
int mgx_iterate_groups(mgx_world *w, uint32_t n_groups, const uint8_t *steps, const uint32_t *step_first);
/* What the per-group schedule calls of this world have done so far: calls that ran MIXED, the sweep-kernel launches of those
 * calls, and the workgroups that sat such a launch out (counted on the host, from the plan).  Equal schedules count nowhere here:
 * they are the plain calls.  Host bookkeeping only: no synchronisation; any pointer may be NULL. */
int mgx_group_schedule_stats(mgx_world *w, uint64_t *mixed_calls, uint64_t *mixed_launches, uint64_t *sat_out);
/* The enabled factor kinds of ONE robot group (ROBOT GROUPS above): kind_mask of MGX_FACTOR_* bits, set before the group's first
 * robot is added.  _get answers what a robot added to the group now would run under. */
int mgx_set_group_enabled(mgx_world *w, uint32_t group, uint32_t kind_mask);
int mgx_get_group_enabled(mgx_world *w, uint32_t group, uint32_t *kind_mask);
/* What the masks have cost so far: schedules (and world-wide fine-grained sweeps) that ran as group plans only because the world
 * is masked, and the sweep-kernel launches of those.  Host bookkeeping only: no synchronisation; either pointer may be NULL. */
int mgx_group_enabled_stats(mgx_world *w, uint64_t *masked_plans, uint64_t *masked_launches);
/* Resident launches for a MASKED world's equal schedules (ROBOT GROUPS above): enabled != 0 switches them on for this world, 0
 * (the default) off.  An ordinary call: it ends a lingering launch first.  _stats: resident launches of the masked form made so
 * far (a launch the residency census declined counts, as in mgx_resident_stats), schedules posted into one (a post taken back
 * does not count), and schedules of the switched-on masked world that ran as group plans all the same.  Host bookkeeping only: no
 * synchronisation; any pointer may be NULL. */
int mgx_set_group_resident(mgx_world *w, int32_t enabled);
int mgx_group_resident_stats(mgx_world *w, uint64_t *launches, uint64_t *posts, uint64_t *fallbacks);
/* The four factor sigmas of ONE robot group (ROBOT GROUPS above), as mgx_params holds the world's: every value finite and > 0, set
 * before the group's first robot is added.  _get answers what a robot added to the group now would run under: the group's own,
 * else the world's. */
typedef struct { double dynamics, interrobot, obstacle, tracking; } mgx_group_sigmas;
int mgx_set_group_sigmas(mgx_world *w, uint32_t group, const mgx_group_sigmas *s);
int mgx_get_group_sigmas(mgx_world *w, uint32_t group, mgx_group_sigmas *out);
/* Batches: several schedules, one submission.  A resident schedule launch pays for itself once — the robots' graphs go
 * HBM -> LDS when it starts and back when it ends, a sixth of a ten-iteration launch at 1000 x 16 — so a caller that issues
 * schedule after schedule with nothing in between (the reference's `iterate_gbp_v2` loop run ahead of the renderer, a planner
 * that looks several ticks ahead, a benchmark loop) brackets the loop: between mgx_batch_begin and mgx_batch_end the schedules
 * handed to mgx_iterate are recorded and submitted TOGETHER, merged into as few launches as their segments fit (32 [external]
 * internal* segments per launch: three ticks of the 10 / 10 schedule) — when the recorded ones fill a launch, at mgx_batch_end,
 * and in front of ANY other call on this world, which therefore finds the world as if every schedule had run when it was issued.
 * Nothing is reordered, nothing skipped: iterate(a); iterate(b) computes what iterate(a ++ b) computes (the phases are
 * flattened either way, robot.rs:1787-1860), bit for bit — the engine's form of capturing a launch-bound loop in a graph.
 * The one visible difference: work recorded in an open batch is on the world's stream only after its submission — a caller that
 * waits on the stream by its own means (events) closes the batch, or calls mgx_synchronize, first.  Works on sharded worlds
 * whose exchange lives in the engine (every rank brackets alike).  n_schedules / n_launches (may be NULL): schedules recorded
 * since mgx_batch_begin and sweep-kernel launches they were submitted as. */
int mgx_batch_begin(mgx_world *w);
int mgx_batch_end(mgx_world *w, uint32_t *n_schedules, uint32_t *n_launches);

/* How the last mgx_iterate / mgx_tick call ran: the number of sweep-kernel launches it enqueued.  A world whose
 * robots all live on this device, with inter-robot factors enabled and few enough robots for every workgroup
 * to be resident at once, runs a whole schedule as ONE launch (robots hand their snapshot records to their
 * neighbours inside it); otherwise one launch per [external iteration] internal* segment.  MGX_PERSISTENT=0 in
 * the environment forces the latter.  Diagnostic (bench.py prices its roofline per launch with it). */
int mgx_last_launch_count(mgx_world *w, uint32_t *n_launches);
/* How the last mgx_iterate / mgx_tick call ran its sweeps, as the launcher that enqueued them chose: the horizon variant of the
 * sweep kernel (K of a constant-K template, 0 / -1 for the run-time-K kernels: K <= 33 / K >= 34), its inter-robot mode
 * (MGX_SWEEP_IR_*), its form (MGX_SWEEP_FORM_*; -1 with ir_mode -1: the call launched no sweep), and how many workgroups of
 * this world's resident instantiation the device holds at once (0: the world's shape has no resident form).  A call that ran
 * several forms (a resident launch the residency census declined, run again launch by launch) reports the last.  Host
 * bookkeeping only: no synchronisation; any pointer may be NULL. */
#define MGX_SWEEP_IR_NONE 0      /* no inter-robot factors */
#define MGX_SWEEP_IR_UNSTAGED 1  /* inter-robot messages read from L2 in every variable sweep (too many edges to stage) */
#define MGX_SWEEP_IR_STAGED 2    /* inter-robot messages staged in LDS */
#define MGX_SWEEP_FORM_SEGMENTS 0  /* one launch per [external iteration] internal* segment */
#define MGX_SWEEP_FORM_RESIDENT 1  /* one resident launch for the schedule */
#define MGX_SWEEP_FORM_POSTED 2    /* posted into a lingering resident launch */
#define MGX_SWEEP_FORM_SHARDED 3   /* one resident launch on a sharded world */
int mgx_last_sweep(mgx_world *w, int32_t *variant, int32_t *ir_mode, int32_t *form, int32_t *resident_capacity);
/* FORMS OF THE RESIDENT KERNEL.  A resident launch runs the smallest instantiation that covers it: without the tracking
 * factors' code where the world's tracking factors are off (MGX_SWEEP_F_TRACKING), without the path of mgx_tick's prior updates
 * where its own schedule carries none and the world has issued no mgx_tick so far (MGX_SWEEP_F_UPDATES).  A lingering launch
 * keeps its form: an mgx_tick that meets a launch without MGX_SWEEP_F_UPDATES ends it and runs as a launch of the covering
 * form, and the world's launches keep that form from then on.  Results are the same bit for bit in every form.
 * A masked world with mgx_set_group_resident on has ONE form, whatever mgx_set_specialize says: the full one with the enabled
 * internal kinds — and, where some group has its own, the factor sigmas (mgx_set_group_sigmas) — read per robot group
 * (MGX_SWEEP_F_GROUP_KINDS | MGX_SWEEP_F_TRACKING | MGX_SWEEP_F_UPDATES = 7).
 * mgx_last_sweep_features: the form of the sweep mgx_last_sweep reports (launch-per-segment kernels: always both bits; 0 as well
 * when no sweep ran).  mgx_set_specialize: 0 = every resident launch of this world in the full form (MGX_SPECIALIZE=0 in the
 * environment does it for the process), 1 = the smallest form, < 0: as the environment says.  For measuring one against the other. */
#define MGX_SWEEP_F_TRACKING 1u
#define MGX_SWEEP_F_UPDATES 2u
#define MGX_SWEEP_F_GROUP_KINDS 4u
int mgx_last_sweep_features(mgx_world *w, uint32_t *features);
int mgx_set_specialize(mgx_world *w, int32_t enabled);
/* How the last neighbour search of this world (mgx_neighbours, mgx_update_topology, a mission tick's) ran, as the branch that
 * launched it chose: the kernel it launched LAST (MGX_SEARCH_*), the row capacity it launched it with (the one-pass kernels write
 * rows of a fixed capacity that the world doubles when a row outgrows it; 0 for the two-pass forms), and how many search launches
 * the call made (1; 2 when a row outgrew the capacity and the search ran again with more room, or when the two-pass forms' rows
 * outgrew the buffer their filling pass guessed and that pass ran again).  n_changed: the one-pass grid kernels of a topology
 * pass say which robots' rows differ from the pass before, and the host's create / delete pass looks at those only — the number of
 * robots so flagged, or -1 where no flags reached that pass (a search outside a topology pass, an all-pairs or two-pass kernel, a
 * search that was run again, a world with removed robots, order keys that do not ascend with the robot ids).  changed (may be
 * NULL): where flags reached it and capacity >= the number of robots, one byte per robot (1: looked at).  Host bookkeeping only:
 * no synchronisation; any pointer may be NULL. */
#define MGX_SEARCH_NONE -1           /* no search since the world was made */
#define MGX_SEARCH_TWO_PASS_PAIRS 0  /* count, scan, fill: all pairs */
#define MGX_SEARCH_TWO_PASS_GRID 1   /* count, scan, fill: hash grid in device memory */
#define MGX_SEARCH_ROWS_PAIRS_4 2    /* one pass, all pairs, four lanes per robot, workgroups of 64 */
#define MGX_SEARCH_ROWS_PAIRS_2 3    /* one pass, all pairs, two lanes per robot, workgroups of 128 */
#define MGX_SEARCH_ROWS_GRID_16 4    /* one pass, hash grid in LDS, rows of up to 16 */
#define MGX_SEARCH_ROWS_GRID_32 5    /* one pass, hash grid in LDS, rows of up to 32 */
#define MGX_SEARCH_ROWS_GROUPS 6     /* one pass, all pairs WITHIN each group (a grouped world, whatever the method) */
int mgx_last_search(mgx_world *w, int32_t *kernel, int32_t *row_cap, int32_t *n_launches, int32_t *n_changed, uint8_t *changed,
                    uint32_t capacity);

/* LINGERING resident launches — schedules issued back to back ride in ONE launch.  The reference's driver runs iterate_gbp_v2
 * tick after tick (robot.rs:85-108, a .chain() in FixedUpdate) with nothing in between but the two prior updates that mgx_tick
 * folds into the launch; a resident launch that ended with its schedule would write every graph back to HBM only for the next
 * one to stage it again (a sixth of a 10-iteration tick at 1000 x 16).  So on an unsharded world a resident launch does not end
 * with its schedule: the robots' workgroups keep their graphs in LDS and wait — at most `microseconds` — for the next mgx_iterate
 * / mgx_tick, which is POSTED into the running launch (a host-mapped box: plan, prior-update records) instead of
 * launched: mgx_last_launch_count reports 1 for it all the same (one submission).  Every other call on the world first ends the
 * launch (it writes back; the call finds the world as after any launch), so nothing observable changes — results are
 * bit-identical, tests/test_gpu_linger.py — except:
 *   * work the CALLER puts on the world's stream behind mgx_iterate / mgx_tick by its own means (events, other kernels) starts
 *     only when the launch has ended: call mgx_flush (ends it, no wait) or mgx_synchronize first;
 *   * a caller that stops issuing schedules without another call leaves the launch waiting out its bound (default 300 us,
 *     MGX_LINGER_US; MGX_LINGER=0 or mgx_set_linger(w, 0): launches end with their schedule).  Every wait inside the launch is
 *     bounded: a host that dies leaves no spinning GPU.
 * A posted schedule the launch did not take any more (it ended first) is run as a launch of its own — nothing lost, nothing
 * twice.  Launches linger only where the calling pattern promises schedules to come (two lingering launches in a row that ended
 * without a post switch it off until schedules are issued back to back again).
 * mgx_linger_stats: launches that lingered, schedules posted into them, posted schedules taken back and re-run (both count
 * SCHEDULES, however many rode in one plan), launches that ended by themselves (waited out their bound) while the host was
 * about to post.
 * mgx_flush: everything issued so far is ENQUEUED — schedules mgx_iterate has recorded (below) are submitted, the launch is told
 * to end — without waiting for the stream.  A caller that shares the world's stream with work of its own flushes first.
 * mgx_set_linger: schedules already recorded are submitted under the old bound first.
 *
 * POST MERGING.  A lingering launch takes post P only when every workgroup has picked up plan P - 2, so a host that issues
 * mgx_iterate back to back soon — from the fourth schedule behind a launch on — waits for the device with the next schedules
 * already in hand.  Instead of waiting, mgx_iterate then records its schedule, and the recorded ones go out TOGETHER as one
 * plan (up to 32 segments: three ticks of the 10 / 10 schedule) — with the first mgx_iterate that finds the post before taken,
 * when one more would not fit, and in front of ANY other call on this world (mgx_tick, every query and read, mgx_flush,
 * mgx_synchronize), which therefore finds the world as if every schedule had run when it was issued.  iterate(a); iterate(b) computes what iterate(a ++ b) computes, bit for bit (batches,
 * above); what is saved is the plan boundary between them: every belief image through HBM and back, three barriers, a poll.
 * The one visible difference: a recorded schedule is on the device only after the caller's NEXT call on the world.  A caller
 * that issues five or more schedules back to back and then goes silent — no flush, synchronize or read — leaves the last ones
 * unsubmitted: the launch (which holds at least two plans of work at that moment) waits out its bound and ends, and the recorded
 * schedules run as a launch with the next call.  Same results, later.  The reference's pattern — one tick, then a read — never
 * has a post outstanding at its next call and is unaffected; mgx_tick is never recorded (its prior updates belong to its first
 * sweep), nor are schedules on sharded worlds (their launches do not linger).
 * mgx_set_post_merge: 0 = off (every schedule its own post, waited for); 1 = automatic (default; MGX_POST_MERGE in the
 * environment, < 0 here: ask it again): record while the post before is untaken, and only schedules that would have been posted
 * on their own; 2 = record whenever a launch lingers and the plan fits, whatever the device has taken, a schedule that opens
 * with an external iteration included behind others — deterministic, for tests and diagnostics.
 * mgx_post_merge_stats: plans posted (mgx_tick's among them, one schedule each; an explicit batch's plan counts as one schedule),
 * schedules in them, schedules in the largest.  Any pointer may be NULL. */
int mgx_flush(mgx_world *w);
int mgx_set_linger(mgx_world *w, int32_t microseconds /* < 0: default (environment) */);
int mgx_linger_stats(mgx_world *w, uint64_t *launches, uint64_t *posts, uint64_t *reruns, uint64_t *ended_by_device);
int mgx_set_post_merge(mgx_world *w, int32_t mode /* 0 off, 1 automatic, 2 always; < 0: default (environment) */);
int mgx_post_merge_stats(mgx_world *w, uint64_t *plans_posted, uint64_t *schedules_in_them, uint64_t *largest);
/* Per-world switch for the above (default: on): 0 keeps every schedule of THIS world on the launch-per-segment path — what
 * MGX_PERSISTENT=0 does for the whole process.  For measuring one against the other; results are identical either way.
 * On a sharded world with resident launches agreed on (mgx_halo_resident_connect_peers) every rank has to switch alike.
 * 2 (diagnostic): on, but this world DECLINES every resident launch — on a sharded world whose ranks agree on every schedule
 * it says no where the others look (mgx_halo_resident_connect_peers), so every rank takes the fall-back; elsewhere like 0. */
int mgx_set_resident_launches(mgx_world *w, int32_t enabled);
/* Whether factors switched back on (mgx_set_enabled) are still taking their first updates from the inboxes they froze with
 * (or inter-robot factors created while their kind was off still lack inbox keys): such schedules run launch by launch.
 * On a sharded world this depends on the flags of the robots THIS rank holds, so the ranks ask each other (any rank still
 * thawing keeps resident launches off on all of them: magics_amd/sharded.py does it after set_enabled). */
int mgx_is_thawing(mgx_world *w, int32_t *thawing);

/* The launch primitive the calls above and below are built on: one device pass per robot
 * that runs the external phases in `external_phases` (bit0 = external factor sweep + routing,
 * bit1 = external variable sweep + routing) and then `n_internal` internal iterations of the
 * phases in `internal_phases` (bit0 = internal factor sweep, bit1 = internal variable sweep;
 * n_internal > 1 needs both).  A sharded driver uses it to place its halo exchange between
 * an internal and the following external phase.  robot = -1: all robots.
 * hints: MGX_HINT_NEXT_STARTS_EXTERNAL — a promise that the next sweep of this world starts with an
 * external factor sweep and that no flag / topology / prior change happens in between; the
 * inter-robot messages computed here are then not stored to HBM (they are recomputed first). */
#define MGX_HINT_NEXT_STARTS_EXTERNAL 1u
int mgx_sweep(mgx_world *w, int32_t robot, uint32_t external_phases, uint32_t internal_phases,
              uint32_t n_internal, uint32_t hints);

/* Fine-grained mirrors of FactorGraph::{internal_factor_iteration,
 * internal_variable_iteration, external_factor_iteration, external_variable_iteration}
 * (factorgraph.rs:688-826).  robot = -1 runs the sweep for every robot.  The external
 * sweeps include the message routing the reference's caller performs
 * (robot.rs:1813-1858) and are only available world-wide (robot must be -1). */
int mgx_internal_factor_iteration(mgx_world *w, int32_t robot);
int mgx_internal_variable_iteration(mgx_world *w, int32_t robot);
int mgx_external_factor_iteration(mgx_world *w, int32_t robot);
int mgx_external_variable_iteration(mgx_world *w, int32_t robot);

/* FactorGraph::change_prior_of_variable + the caller's routing to external factors
 * (factorgraph.rs:494-528, variable.rs:203-230, robot.rs:2262-2282). */
int mgx_change_prior(mgx_world *w, int32_t robot, uint32_t var_ix, const double mean[4]);
/* batched form: n triples (robot[i], var_ix[i], means[i][4]) in one launch */
int mgx_change_priors(mgx_world *w, uint32_t n, const int32_t *robots, const uint32_t *var_ix,
                      const double *means);

/* FactorGraph::reset_variables(&means, first_last_sigma, inbetween_sigma) (factorgraph.rs:1541-1564; VariableNode::reset,
 * variable.rs:350-360; FactorNode::empty_inbox, factor/mod.rs:480-483) for one robot's graph: every variable's belief mean
 * becomes means[i] and its belief precision diag(sigma) — first_last_sigma for variables 0 and K-1, inbetween_sigma for the
 * others, used as the reference uses them (AS the diagonal, +inf allowed) — and every message in the variables' inboxes and
 * in the inboxes of the graph's own factors becomes empty.  means: [n_means][4]; n_means must equal the graph's number of
 * variables K (the reference asserts it, factorgraph.rs:1548: MGX_ERR_INVALID otherwise, nothing read).  mgx_reset_tracking_factors:
 * FactorGraph::reset_tracking_factors (factorgraph.rs:1566-1590) — the graph's tracking factors skip their next ten
 * updates (tracking.rs:153-155,362-371).  The reference calls the pair (means, 1e30, +inf) when a global path arrives
 * (robot.rs:766-769); rare, so the engine re-lays the device state out on the next launch. */
int mgx_reset_variables(mgx_world *w, int32_t robot, const double *means, uint32_t n_means, double first_last_sigma,
                        double inbetween_sigma);
int mgx_reset_tracking_factors(mgx_world *w, int32_t robot);
/* FactorGraph::modify_tracking_factors(|t| t.set_tracking_path(path)) (factorgraph.rs:1467, tracking.rs:134-136): the first of
 * the three calls of the path-finding completion handler (robot.rs:674-682, then reset_variables and reset_tracking_factors,
 * robot.rs:766-769).  Every tracking factor of the robot's graph follows the new polyline from its next update on and keeps
 * its record, its last measurement and its timeout: a factor whose record is already >= n_path - 1 is skipped from then on
 * (tracking.rs:373-379), a robot added without a path starts tracking.  path_xy: [n_path][2] f32, 2 <= n_path <= 65535
 * (TwoOrMore; the engine keeps a factor's record in 16 bits beside its timeout); the robot must be a live local one
 * (MGX_ERR_INVALID otherwise, nothing changes).  Only the packed path arrays are rebuilt
 * and uploaded: no state is pulled, nothing else is laid out again. */
int mgx_set_tracking_path(mgx_world *w, int32_t robot, const float *path_xy, uint32_t n_path);
/* The whole path-finding completion handler (robot.rs:643-799) for a batch of robots in ONE call — global paths arrive in bursts
 * (a formation that spawns, a fleet that re-plans).  For every listed robot i, in the handler's order and with the same arguments:
 *   mgx_set_tracking_path(robots[i], path_i)                                   robot.rs:674-682
 *   mgx_reset_variables(robots[i], means[i], K, first_last_sigma, inbetween_sigma)   robot.rs:766-768
 *   mgx_reset_tracking_factors(robots[i])        if MGX_GLOBAL_PATH_RESET_TRACKING   robot.rs:769
 *   Route::update_waypoints(path_i)              if MGX_GLOBAL_PATH_ROUTE            robot.rs:778, :389-392
 *   mgx_set_idle(robots[i], 0)                   if MGX_GLOBAL_PATH_ACTIVATE         robot.rs:786
 * path_i = path_xy[path_ptr[i] .. path_ptr[i+1]) ([.][2] f32, 2 <= points <= 65535); means: [n][K][4].  With ROUTE the robot's
 * device mission (mgx_mission_set) takes the route path_i[1:] widened to f64 — target_index = 1 skips the first point — and its
 * next waypoint is that route's first; reach rules, Transform and time scale stay.
 * Refused as a whole, nothing changed: null arrays, a path outside 2 .. 65535 points, a robot that is not a live local one or
 * is listed twice (MGX_ERR_INVALID); ROUTE on a robot without a mission or whose mission is complete (MGX_ERR_STATE) — a robot
 * that waits between two legs (mgx_mission_legs_ended) is not complete: this call is its hand-over.
 * Which worlds take which path:
 *   - laid out (launched at least once, no robot / obstacle change pending), unsharded, and in none of the switching states
 *     (no factor kind ever switched at run time, no factors that still lack inbox keys): applied IN PLACE on the device by one
 *     small kernel pair — nothing is pulled, nothing is laid out again (mgx_layout_stats does not move);
 *   - every other world (not laid out yet or about to be laid out again, sharded, a kind switched with mgx_set_enabled): the
 *     per-robot calls above run internally — the same result, at the price of one re-layout by the next launch. */
#define MGX_GLOBAL_PATH_RESET_TRACKING 1u  /* reset_tracking_factors          robot.rs:769                 */
#define MGX_GLOBAL_PATH_ROUTE          2u  /* active_route.update_waypoints   robot.rs:778, :389-392       */
#define MGX_GLOBAL_PATH_ACTIVATE       4u  /* mission.state = Active          robot.rs:786  (idle := 0)     */
int mgx_apply_global_paths(mgx_world *w, uint32_t n, const int32_t *robots, const uint32_t *path_ptr, const float *path_xy,
                           const double *means, double first_last_sigma, double inbetween_sigma, uint32_t flags);
/* Which path ran (read-only, no side effect on launches in flight): n_layouts counts the full rebuilds of the device arrays
 * from the host mirror, n_pulls the downloads of the device state into it, since the world was created.  Either may be null. */
int mgx_layout_stats(mgx_world *w, uint64_t *n_layouts, uint64_t *n_pulls);
/* Head-room for robots that join a running world (the reference's spawner, spawner.rs:415-646, builds a RobotBundle —
 * robot.rs:1134-1356 — for as long as a formation repeats).  The world expects to hold up to `robots` robots, removed ones
 * included: the next full layout sizes every per-robot device array, and strides the tables keyed by (robot, factor), for that
 * many, and from then on the robots mgx_robot_add brings are APPENDED on the device by the next call that needs it — one staged
 * block and one kernel for all robots added since, nothing pulled, nothing laid out again (mgx_layout_stats does not move, the
 * resident launches' capacity and the neighbour search's buffers stay).  Callable at any time: before the first layout the
 * wish is only recorded; on a laid-out world it costs ONE full layout and one pull, by the next launch.  A value at or below
 * the current robot count, or below an earlier wish, keeps the head-room already there; 0 on a world that never reserved
 * is a no-op.  A world that never calls this keeps the layout, the strides and the add path it always had.
 * The append is taken when nothing but additions is pending, the world is unsharded and the new robots are no ghosts, no factor
 * kind was ever switched at run time (mgx_set_enabled) and no factor lacks inbox keys, and the robots and their paths fit
 * the head-room; anything else — ghosts and sharded worlds accept the call and never append — is laid out in full as before,
 * with the same results.  Robots beyond the head-room: one full layout sized max(robots asked for, 2 x robots there). */
int mgx_world_reserve(mgx_world *w, uint32_t robots);
/* Which path the additions took (read-only, as mgx_layout_stats): `appends` counts the commits that appended in place,
 * `robots_appended` the robots they brought onto the device, `fallbacks` the commits of a reserved, already laid-out world
 * that had new robots and ran the full layout all the same.  Any may be null; a null world: -1, nothing written. */
int mgx_append_stats(mgx_world *w, uint64_t *appends, uint64_t *robots_appended, uint64_t *fallbacks);

/* The driver's per-tick prior updates, batched over robots in one launch:
 *   what[i] & 1: update_prior_of_horizon_state (robot.rs:2182-2283) — the last variable of robots[i]
 *                moves towards waypoints_xy[i] at min(max_speed, distance) for delta_t seconds;
 *   what[i] & 2: update_prior_of_current_state_v3 (robot.rs:2286-2338) — variable 0 moves by
 *                time_scale[i] * (mean_1 - mean_0), time_scale = fixed_dt / t0 (an f32 quotient widened).
 * Each ends in change_prior of that variable.  The caller lists the robots the reference's systems would
 * not skip (not idle / not finished / with a next waypoint) and keeps the mission logic. */
int mgx_update_priors(mgx_world *w, uint32_t n, const int32_t *robots, const double *waypoints_xy,
                      const double *time_scale, const uint8_t *what, double max_speed, double delta_t);
/* One FixedUpdate tick of the planner chain in one call: the two prior updates above for the listed
 * robots, then iterate_gbp_v2 over `steps` (robot.rs:86-103).  Same results as mgx_update_priors
 * followed by mgx_iterate; when the schedule opens with an internal iteration (every schedule of the
 * reference does) the prior updates are applied inside the launch that runs it, on the image each
 * robot's workgroup has just staged, instead of by a kernel of their own. */
int mgx_tick(mgx_world *w, uint32_t n, const int32_t *robots, const double *waypoints_xy,
             const double *time_scale, const uint8_t *what, double max_speed, double delta_t,
             const uint8_t *steps, uint32_t n_steps);

/* ---- whole driver ticks on the device -----------------------------------------------------
 * The rest of the reference's FixedUpdate chain around iterate_gbp_v2 (robot.rs:86-103) with its state on the device, so
 * that a tick costs the host ONE synchronisation (the neighbour rows the connection bookkeeping needs) instead of four
 * belief read-backs: a robot's mission — its route, the next waypoint, the reached-when rules of formation.yaml and the
 * Bevy Transform it moves — is handed over once (mgx_mission_set); every mgx_mission_tick then runs
 *   reached_waypoint                         robot.rs:2080-2176  estimated position (belief mean of the rule's variable, as f32)
 *                                                                against the next waypoint, f32 squared distance; the last
 *                                                                waypoint completes the mission (and despawns the robot,
 *                                                                robot.rs:2172, when despawn_finished is set)
 *   update_robot_neighbours + delete_ / create_interrobot_factors   robot.rs:1362-1586  on the device's Transforms, exactly
 *                                                                mgx_update_topology otherwise
 *   update_failed_comms                      robot.rs:1593-1601  `antennas` (one byte per robot id, the caller's draws; NULL: none)
 *   update_prior_of_horizon_state / _current_state_v3 + the Transform increment   robot.rs:2182-2338
 *   iterate_gbp_v2                           robot.rs:1769-1861  over `steps`
 * stats (optional) = {connections created, pairs deleted, missions completed this tick}.  Unsharded worlds.
 * A robot whose mission is idle (mgx_set_idle: MissionState::Idle, waiting for a global path) waits: its next waypoint does not
 * advance (Mission::advance_to_next_waypoint, robot.rs:995-1005), it gets no prior update and its Transform does not move
 * (both systems skip it, robot.rs:2212, 2303); it still takes part in the neighbour search, the topology pass and the collision
 * passes, and sits out the sweeps.  mgx_apply_global_paths with MGX_GLOBAL_PATH_ROUTE | MGX_GLOBAL_PATH_ACTIVATE hands it its
 * route and wakes it up.
 *
 * MISSIONS OF SEVERAL LEGS.  The reference's global-planner mission keeps all its taskpoints (Mission::global, robot.rs:862-908)
 * and follows one planned route per pair of them: when a route ends with taskpoints left, Mission::next_route (robot.rs:966-993)
 * does not complete the mission — it opens the route [taskpoint k, taskpoint k+1] and sets MissionState::Idle, progress_missions
 * (robot.rs:578-633) plans it, and the completion handler (robot.rs:643-799) wakes the robot on the new path.  Here the device
 * knows how many legs follow the route it holds (mgx_mission_desc.legs_after -> legs_left, an int32 per robot that the device
 * counts down) and the HOST plans and hands over, as it does at spawn:
 *   - a robot reaches the last waypoint of its route under the FINISH rule on every leg (Mission::next_waypoint_is_last is true
 *     on the last waypoint of the newest route, robot.rs:943-948, 2119-2123);
 *   - with legs_left > 0 that ends a LEG: legs_left -= 1, the mission is NOT complete (finished_tick stays -1), the next
 *     waypoint index stays == the route's length — so the robot gets no prior update and its Transform does not move — and
 *     the robot is reported beside the completions at the tick's one synchronisation;
 *   - mgx_mission_tick_begin (every form) makes it idle (as mgx_set_idle(robot, 1): the flags and edge gates travel ahead of
 *     this tick's sweeps and of its message counters) and lists it in mgx_mission_legs_ended, ascending ids, until the next
 *     _begin.  It is not despawned, not counted in stats[2] and not listed by mgx_mission_finished; the grouped forms need
 *     nothing more — the robot ids say which group;
 *   - mgx_apply_global_paths with MGX_GLOBAL_PATH_ROUTE | MGX_GLOBAL_PATH_ACTIVATE is the hand-over of the next leg, exactly as
 *     at spawn and in place where the world allows (mgx_layout_stats does not move): the route becomes path[1:], the next
 *     waypoint its first, the robot Active; legs_left is not touched;
 *   - with legs_left == 0 the route's end completes the mission: everything as without legs.
 * While it waits the robot is idle and therefore not evaluated by reached_waypoint.  Missions do not migrate and sharded worlds
 * have none, as before. */
typedef struct mgx_mission_desc {
    uint32_t n_waypoints;         /* waypoints still to visit; the first one is the next target (>= 1)                 */
    uint32_t legs_after;          /* further legs that follow this route (MISSIONS OF SEVERAL LEGS below); 0: the route's
                                     last waypoint completes the mission (a word that was reserved and 0)              */
    const double *waypoints_xy;   /* [n][2]; compared as f32 (the reference's Vec2), used as f64 by the horizon prior   */
    uint32_t reach_var, finish_var;   /* variable tested against an intermediate / the final waypoint: 0 = current,
                                         K-1 = horizon (waypoint-reached-when-intersects / finished-when-intersects)   */
    float reach_dist2, finish_dist2;  /* squared distance limits in f32 (robot-radius^2 or meter^2)                    */
    float translation[3];         /* Transform::translation at hand-over (x, height, y)                                */
    float reserved2;
    double time_scale;            /* fixed_dt / t0 as the f32 quotient widened (robot.rs:2309)                         */
} mgx_mission_desc;
int mgx_mission_set(mgx_world *w, int32_t robot, const mgx_mission_desc *desc);
int mgx_mission_tick(mgx_world *w, float comms_radius, uint32_t method, uint64_t *robot_number_next,
                     int32_t despawn_finished, const uint8_t *antennas, double max_speed, double delta_t,
                     const uint8_t *steps, uint32_t n_steps, uint32_t *stats);
/* The tick in two halves, for a caller whose comms-failure draws depend on which robots are still alive after this tick's
 * despawns (the reference draws once per live robot, robot.rs:1599): _begin runs reached_waypoint and the topology pass (the
 * tick's one synchronisation) and leaves the robots whose mission completed in mgx_mission_finished (ascending ids);
 * _end applies the antennas, the prior updates with the Transform increment and the schedule.  Robots may be added (and
 * given missions) between the halves.  mgx_mission_tick == _begin + _end. */
int mgx_mission_tick_begin(mgx_world *w, float comms_radius, uint32_t method, uint64_t *robot_number_next,
                           int32_t despawn_finished, uint32_t *stats);
int mgx_mission_tick_end(mgx_world *w, const uint8_t *antennas, double max_speed, double delta_t,
                         const uint8_t *steps, uint32_t n_steps);
/* mgx_mission_tick_begin with one RobotNumberGenerator per group (ROBOT GROUPS; arguments as mgx_update_topology_groups): stats
 * (optional) [n_groups][3] = {connections created, pairs deleted, missions completed this tick} per group.  Paired with
 * mgx_mission_tick_end; mgx_mission_finished lists the robots of all groups, ascending ids. */
int mgx_mission_tick_begin_groups(mgx_world *w, float comms_radius, uint32_t method, uint32_t n_groups, uint64_t *number_next,
                                  int32_t despawn_finished, uint32_t *stats);
/* ... and one comms radius per group: comms_radii [n_groups], by group id.  A radius that is not the one of the tick before
 * discards the rows that tick's _end searched ahead: this tick searches again, with the new radii. */
int mgx_mission_tick_begin_groups_radii(mgx_world *w, const float *comms_radii, uint32_t method, uint32_t n_groups,
                                        uint64_t *number_next, int32_t despawn_finished, uint32_t *stats);
/* mgx_mission_tick_end with one schedule per robot group in place of the one `steps` (ROBOT GROUPS above; arguments as
 * mgx_iterate_groups).  Pairs with any of the _begin forms. */
int mgx_mission_tick_end_groups(mgx_world *w, const uint8_t *antennas, double max_speed, double delta_t,
                                uint32_t n_groups, const uint8_t *steps, const uint32_t *step_first);
int mgx_mission_finished(mgx_world *w, int32_t *robots, uint32_t capacity, uint32_t *n);
/* The robots that ended a leg with legs left in the last _begin (MISSIONS OF SEVERAL LEGS above), ascending ids, all groups:
 * *n = how many, the first min(*n, capacity) of them in `robots` (may be NULL).  No synchronisation: _begin's own lies behind. */
int mgx_mission_legs_ended(mgx_world *w, int32_t *robots, uint32_t capacity, uint32_t *n);
/* MANY ticks in one call: what a headless run does between two spawns (the reference's FixedUpdate chain tick after tick,
 * robot.rs:85-108, with update_failed_comms' draws in between) without the caller's interpreter in the loop —
 *   for each tick:  mgx_mission_tick_begin;  one Bernoulli(failure_rate) draw per robot alive after the tick's despawns, id
 *                   order, from the caller's WyRand stream (rand 0.8.5 Bernoulli over wyrand 0.2.0, restated in
 *                   magics_amd/prng.py: one u64 per draw unless failure_rate == 1; wyrand_state NULL: no stream, no draws);
 *                   mgx_mission_tick_end (the draws as antennas when failure_rate > 0).
 * Per tick t < ticks_done the caller gets what it would have seen tick by tick: connections created / pairs deleted, the
 * number of missions completed and, one after the other in `finished`, the robots concerned (ascending within a tick), the
 * Transform::translation of EVERY robot after the tick's move ([n_ticks][n_robots][3], may be NULL) and the draws
 * ([n_ticks][n_robots], 1 = on air, may be NULL).  stop_when_all_finished: returns behind the tick that completed the last
 * mission.  No robot may join during the call.  Identical to the same ticks issued one by one (tests/test_gpu_sim.py).
 * The call also returns behind the first tick in which a robot ended a leg with legs left (MISSIONS OF SEVERAL LEGS): ticks_done
 * says where, mgx_mission_legs_ended whose — the caller plans the next leg and calls again.  Such a robot is unfinished for
 * stop_when_all_finished.  A world without legs never sees this.
 * ONE generator and ONE draw stream, also on a grouped world (ROBOT GROUPS): per-group many-tick runs are not part of this call. */
typedef struct mgx_mission_run_desc {
    uint32_t n_ticks;
    float comms_radius;
    uint32_t method;                  /* MGX_NEIGHBOURS_* */
    int32_t despawn_finished, stop_when_all_finished;
    uint32_t n_steps;
    const uint8_t *steps;
    double max_speed, delta_t, failure_rate;
    uint64_t *wyrand_state;           /* in / out */
    uint64_t *robot_number_next;      /* in / out */
    uint32_t *created, *deleted, *n_finished; /* out [n_ticks] */
    int32_t *finished;                /* out [finished_capacity] */
    uint32_t finished_capacity;
    uint32_t finished_total;          /* out */
    float *translations;              /* out [n_ticks][n_robots][3] or NULL */
    uint8_t *antennas;                /* out [n_ticks][n_robots] or NULL */
    uint32_t ticks_done;              /* out */
    uint32_t reserved;
} mgx_mission_run_desc;
int mgx_mission_run(mgx_world *w, mgx_mission_run_desc *desc);
/* Transform::translation [n][3] of every robot as of the end of the last tick, WITHOUT synchronising: _end sends them to
 * the host behind its launches, so they are complete once the stream has been synchronised since — which the next
 * mgx_mission_tick_begin does by itself.  (PositionTracker / VelocityTracker samples, planner/tracking.rs:104-218.) */
int mgx_mission_translations(mgx_world *w, float *translations, uint32_t capacity_robots, uint32_t *n_robots);
/* Transform::translation [n][3], next waypoint index (== the route's length once complete; -1: no mission) and the tick
 * at which each mission completed (-1 before) of every robot, id order; any pointer may be NULL.  Synchronises. */
int mgx_mission_read(mgx_world *w, float *translations, int32_t *targets, int64_t *finished_tick);
/* legs_left [n] of every robot, id order (0: no mission, or none left), as the device has counted them down.  Synchronises
 * as mgx_mission_read does. */
int mgx_mission_legs_read(mgx_world *w, int32_t *legs_left);

/* ---- robot-robot collision bookkeeping on the device -------------------------------------------------------
 * update_robot_robot_collisions with the Free / Colliding state machine of CollisionHistory (planner/collisions.rs:72-140,
 * 455-495), the figure the reference's export is read for next to makespan and smoothness.  One PASS looks at the robots
 * alive at that moment (not removed, not ghosts), their Transforms (x, z) as f32 and r = (float)desc.radius:
 *   pair (a, b), a < b by robot id, overlaps iff dx*dx + dy*dy <= (r_a + r_b)*(r_a + r_b), d = p_b - p_a, every operation
 *   rounded to f32 on its own (the same in libmgx.so and libmgx_fma.so); a NaN anywhere: no overlap;
 *   a pair that overlaps now and did not in the pass before (or was not looked at: one of the two was not alive, or is new)
 *   is one collision EVENT, with mins = max(p_a - r_a, p_b - r_b), maxs = min(p_a + r_a, p_b + r_b) per axis (the
 *   intersection of the two balls' AABBs), and counts once for robot a and once for robot b;
 *   a pair that parts, or loses a robot, is Free again.  Events of despawned robots stay in the log.
 * Robot-environment collisions are a pass of their own (mgx_env_collisions_*, below the environment rasteriser).
 * mgx_collisions_enable(w, 1, method, event_capacity): switches the bookkeeping on (default: off — no kernel, no allocation).
 *   method: MGX_NEIGHBOURS_AUTO / _PAIRS / _GRID (all pairs below 512 alive robots, a hash grid of 2 r_max cells above; the same
 *   events either way).  event_capacity (0: 262144) records of log and room for 65536 pairs overlapping at once are allocated
 *   here and never grow.  Calling it again while on changes the method only; (w, 0, ..) switches off and drops the state.
 * While on, every mgx_mission_tick_end (so every mgx_mission_tick and every tick of mgx_mission_run) enqueues one pass on the
 *   Transforms after that tick's move and the robots alive after that tick's despawns, in front of the schedule's launches:
 *   no synchronisation, nothing read back.
 * mgx_collisions_update: the same pass over positions the caller keeps ([n_robots][3], x and z are read; NULL: the device's
 *   mission Transforms as they are) — the mgx_update_topology counterpart.  Enqueued, not waited for.
 * mgx_collisions_read: the one call that synchronises.  events [first, first + capacity) of the log in (pass, robot_a, robot_b)
 *   order (pass: 0 for the first pass since enable / clear), *n_total = events in the log, *dropped = events that found the
 *   log full (counted, not stored; the per-robot counts include them), per_robot [n_robots] (may be NULL) = contacts of every
 *   robot.  Nothing is lost silently: if more pairs overlapped at once than there is room for, the call fills its outputs and
 *   returns MGX_ERR_STATE (later passes may have missed contacts).
 * mgx_collisions_clear: clear_robot_robot_collisions (collisions.rs:68-70): everybody Free, log and counts empty, pass 0.
 * Unsharded worlds (MGX_ERR_STATE on a world with ghosts); MGX_ERR_STATE from _update / _read / _clear while switched off. */
typedef struct mgx_collision_event {
    uint64_t pass;
    int32_t robot_a, robot_b;     /* robot_a < robot_b */
    float mins[2], maxs[2];       /* (x, z) */
} mgx_collision_event;
int mgx_collisions_enable(mgx_world *w, int32_t enabled, uint32_t method, uint64_t event_capacity);
int mgx_collisions_update(mgx_world *w, const float *positions_xyz);
int mgx_collisions_read(mgx_world *w, uint64_t first, mgx_collision_event *events, uint64_t capacity, uint64_t *n_total,
                        uint64_t *dropped, uint32_t *per_robot);
int mgx_collisions_clear(mgx_world *w);

/* ---- read-back ----------------------------------------------------------------------- */
/* VariableNode.belief (variable.rs:40-54).  Any output pointer may be NULL. */
int mgx_get_belief(mgx_world *w, int32_t robot, uint32_t var_ix, double eta[4], double lam[16],
                   double mean[4], double cov[16], int32_t *valid);
/* bulk: robots in id order, variables in index order; ghosts are skipped.
 * means [sum K][4]; eta [sum K][4]; lam [sum K][16].  Any pointer may be NULL. */
int mgx_read_beliefs(mgx_world *w, double *eta, double *lam, double *means);
/* means only — what reached_waypoint (robot.rs:2125-2136) and the visualisers read per tick */
int mgx_read_means(mgx_world *w, double *means);
/* the mean of ONE variable of every robot, [n_robots][4]: nth_variable(0) / last_variable for
 * reached_waypoint (robot.rs:2125-2136), variables 0 and 1 for the Transform increment of
 * update_prior_of_current_state_v3 (robot.rs:2309-2330) — 32 bytes per robot instead of 32 K */
int mgx_read_variable_means(mgx_world *w, uint32_t var_ix, double *means);
int mgx_num_robots(mgx_world *w, uint32_t *n_robots, uint32_t *n_variables);
/* FactorGraph::messages_sent() / messages_received() (factorgraph.rs:876-890; MessageCount,
 * factorgraph/mod.rs:29-137) of one robot's graph, as exported by export.rs:434-439:
 * counts = {sent internal, sent external, received internal, received external}, summed over the
 * nodes the graph holds now (a deleted inter-robot factor takes its counts with it).  The counts
 * depend only on topology, enabled kinds, antenna / idle flags and iteration counts, so they are
 * kept on the host (launches are logged, no device work). */
int mgx_message_counts(mgx_world *w, int32_t robot, uint64_t counts[4]);
/* Sharded worlds keep the counters too (for the robots a rank OWNS), provided the rank's mirror holds every connection a
 * local robot takes part in — also the ones it owns towards robots of other ranks (mgx_ir_connect with a ghost target:
 * bookkeeping only, no device edge) — and is told the prior changes other ranks apply to its ghosts: */
int mgx_note_change_priors(mgx_world *w, uint32_t n, const int32_t *robots, const uint32_t *var_ix);

/* ---- multi-GPU halo (one exchange per external iteration) ----------------- */
/* Number of f64 words of one robot's halo record with K variables. */
uint32_t mgx_halo_words(uint32_t K);
/* Register the exchange lists once: the local robots whose snapshot records are written
 * to the send buffer (in this order) and the ghost robots filled from the receive buffer. */
int mgx_halo_plan(mgx_world *w, uint32_t n_send, const int32_t *send_robots, uint32_t n_recv,
                  const int32_t *recv_ghosts);
/* The same lists derived from the connections this world holds, for a sharded world that FOLLOWS its
 * topology: every rank holds every robot (its own ones and ghost copies of all the others, ids equal
 * on all ranks), runs mgx_update_topology on all positions — the bookkeeping of robot.rs:1386-1586 is
 * then replicated, identical everywhere — and exchanges the snapshot records of exactly those robots
 * that own a connection into a robot of another rank.  rank_of[robot] = owning rank; the lists are
 * grouped by peer rank, ascending robot id inside a group, and both ends of every exchange derive
 * matching groups.  send_counts / recv_counts [n_ranks]: records per peer.  Call after every topology
 * pass that changed something, then exchange once (pack / all-to-all-v / unpack) BEFORE the next
 * sweep: the factors the pass created take the owner's delivery count of that exchange as their
 * creation epoch.  Host-driven transports only (the direct / RCCL wirings are per plan). */
int mgx_halo_plan_from_connections(mgx_world *w, const int32_t *rank_of, uint32_t n_robots,
                                   int32_t my_rank, uint32_t n_ranks, uint32_t *send_counts,
                                   uint32_t *recv_counts);
/* The sharding plan itself (host only, no device; identical on every rank, no communication):
 * mgx_shard_partition — owner rank of every robot: contiguous strips in (y, x) order of the robots' positions with equal
 *   robot counts (spatial blocks keep cross-rank pairs few); ties broken by robot index.
 * mgx_shard_plan_create — one rank's view, from the owner map and the directed connections (owner robot a, other robot
 *   b) of create_interrobot_factors (robot.rs:1490-1541): the local robots, the ghosts (owners of connections whose
 *   target is local), the indices of the connections evaluated here, and per peer rank q the robots whose snapshot
 *   records go to q / arrive from q — segments [first[q], first[q+1]) of the send / receive lists, ascending robot id
 *   inside a segment, i.e. exactly the order mgx_halo_plan and the transports expect.
 * mgx_shard_plan_counts sizes the arrays of mgx_shard_plan_get (first arrays: n_ranks + 1 entries); any output may be NULL. */
typedef struct mgx_shard_plan mgx_shard_plan;
int mgx_shard_partition(const double *positions_xy, uint32_t n_robots, uint32_t n_ranks, int32_t *owner);
int mgx_shard_plan_create(const int32_t *owner, uint32_t n_robots, const int32_t *conn_owner,
                          const int32_t *conn_other, uint32_t n_conns, int32_t rank, uint32_t n_ranks,
                          mgx_shard_plan **out);
void mgx_shard_plan_destroy(mgx_shard_plan *plan);
int mgx_shard_plan_counts(const mgx_shard_plan *plan, uint32_t *n_local, uint32_t *n_ghosts,
                          uint32_t *n_connections, uint32_t *n_send, uint32_t *n_recv);
int mgx_shard_plan_get(const mgx_shard_plan *plan, int32_t *local, int32_t *ghosts, uint32_t *connections,
                       uint32_t *send_first, int32_t *send_robots, uint32_t *recv_first,
                       int32_t *recv_robots);

/* Pack the planned robots' variable->own-factor snapshots (what their inter-robot factors on
 * other ranks read) into `dev_buf` (device pointer, n_send records of mgx_halo_words(K) f64),
 * resp. unpack n_recv records into the ghost robots.  Asynchronous on the world's stream. */
int mgx_halo_pack(mgx_world *w, void *dev_buf);
int mgx_halo_unpack(mgx_world *w, const void *dev_buf);

/* ---- migration: a robot changes its owning rank (worlds that follow their topology) --------------------------------------
 * The reference has ONE world and no notion of ownership (robot.rs queries run over every entity); a sharded world that
 * follows its topology re-balances by moving a robot's graph between ranks.  Everything that exists on the owner's rank
 * only travels in one flat, self-describing record: the graph's numeric state (priors, beliefs, factor -> variable
 * messages, snapshot records and delivery counts, tracking records, iteration count, path, frozen inboxes), the totals of
 * its MessageCount, and the state of every InterRobotFactor attached to its variables (kept at the target's rank).  The
 * replicated bookkeeping (connection sets, node slots, robot numbers, flags, the connections' counters) stays where it is.
 * Protocol, on every rank at the same point BETWEEN ticks (after the sweeps that followed the last mgx_update_topology):
 *   old owner:  mgx_robot_export (bytes first with buf = NULL, then the record), mgx_robot_release
 *   new owner:  mgx_robot_import with the record (refused with MGX_ERR_STATE when its connections differ from this
 *               rank's bookkeeping: the ranks' topology passes are out of step)
 *   every rank: the new rank table to mgx_halo_plan_from_connections, and the in-engine transports wired again (device
 *               indices change: locals first) — as after mgx_robot_add.
 * What does NOT travel: device-side missions (mgx_mission_*: routes, next waypoints, Transforms, completion ticks are state of
 * unsharded worlds, device index == robot id).  Export, import and release of a robot that has one are refused (MGX_ERR_STATE).
 * Results stay bit-identical to the unsharded world's (tests/test_gpu_sharded.py::test_robots_migrate_between_ranks). */
int mgx_robot_export(mgx_world *w, int32_t robot, void *buf, uint64_t capacity, uint64_t *bytes);
int mgx_robot_import(mgx_world *w, int32_t robot, const void *buf, uint64_t bytes);
int mgx_robot_release(mgx_world *w, int32_t robot);

/* ---- halo exchange through RCCL inside the library -------------------------------------------
 * pack -> grouped ncclSend / ncclRecv with every peer (the all-to-all-v of boundary snapshots over
 * xGMI) -> unpack, enqueued on the world's stream in front of every world-wide launch
 * that starts with the external factor phase: no host work per exchange beyond the enqueue.  RCCL
 * is resolved at run time (dlopen; the copy already in the process if there is one).  One rank
 * creates the id (mgx_rccl_unique_id), all ranks get it over any control plane and call
 * mgx_halo_rccl_connect (collective: ncclCommInitRank) with their peers and the segments of the
 * send / receive lists (mgx_halo_plan) that belong to each. */
int mgx_rccl_unique_id(uint8_t id[128]);
int mgx_halo_rccl_connect(mgx_world *w, const uint8_t id[128], uint32_t n_ranks, uint32_t rank,
                          uint32_t n_peers, const uint32_t *peer_rank, const uint32_t *send_first,
                          const uint32_t *recv_first);
int mgx_halo_rccl_disconnect(mgx_world *w);

/* ---- direct halo exchange: peer-mapped stores instead of the collective -------
 * Same dataflow as pack -> all-to-all-v -> unpack, without a collective and without host work
 * per exchange: each producer's kernel stores its boundary records straight into the consumer
 * rank's receive area over xGMI and then bumps an arrival counter there; the consumer's kernel
 * waits for the counters of all its producers and fills its ghost robots.  Once connected, every
 * world-wide launch that starts with the external factor phase (mgx_iterate, mgx_sweep,
 * mgx_external_factor_iteration) runs the exchange first, asynchronously on the world's stream.
 * All ranks must issue the same sequence of such launches (they do: one schedule).
 *
 * The wiring is made ONCE and outlives changes of the exchange lists (a world that follows its topology: connections across
 * ranks come and go with robot.rs:1386-1586, mgx_update_topology + mgx_halo_plan_from_connections); a rank's PEERS are the ranks
 * it shares a boundary with (fixed lists: those it sends to, which are those it receives from — inter-robot factors come in
 * pairs, robot.rs:1490-1541) or every other rank (lists that change).  After mgx_halo_plan* (send list grouped by consumer,
 * receive list grouped by producer):
 *   1. mgx_halo_direct_setup_slots: allocates this rank's receive area — `slot_capacity` record slots per parity, one per ghost
 *      robot of this rank, slot = the robot's place among the rank's ghosts in device order (mgx_halo_ghost_slots; capacity >=
 *      their number, room for robots that join), fine-grained device memory — and one arrival counter per peer
 *      (n_sources = number of peers); returns their device addresses.  Every peer is a source with or without records in an
 *      exchange: a rank that sends nothing still publishes the exchange number, a rank that receives nothing still waits for
 *      all of them (that wait is its flow control: nobody gets two exchanges ahead of anybody).
 *   2. the ranks swap these addresses — mgx_ipc_export / mgx_ipc_open across processes (hipIpc*), raw pointers inside one
 *      process — together with the area's capacity, the slot of every robot in it, and per producer the address of its counter
 *      (flag_base + 8 * index of the producer among the consumer's peers).
 *   3. mgx_halo_direct_connect_slots, and again after every change of the lists, (re)aims the pushes — peers in the order of the
 *      send list's segments (send_first: one per peer, possibly empty), for every entry of the send list the slot of that robot
 *      in its consumer's area.  Exchange numbers go on across calls.  The aim outlives a relayout that keeps the robots' device
 *      order (new obstacles, reset variables); a robot that joins, migrates or is released takes it away, and an exchange is
 *      refused (MGX_ERR_STATE) until the pushes are aimed again.
 * A wait that exceeds MGX_HALO_TIMEOUT_MS (default 5000) gives up, leaves the ghosts untouched
 * and is reported by mgx_halo_direct_status (never a hung GPU). */
int mgx_halo_direct_setup_slots(mgx_world *w, uint32_t n_sources, uint32_t slot_capacity, void **recv_base, void **flag_base);
int mgx_halo_ghost_slots(mgx_world *w, uint32_t n, const int32_t *robots, int32_t *slots);
/* the exchange lists as they stand (robot ids, by peer rank in the order of mgx_halo_plan_from_connections' counts) */
int mgx_halo_get_lists(mgx_world *w, int32_t *send_robots, uint32_t send_capacity, int32_t *recv_robots, uint32_t recv_capacity,
                       uint32_t *n_send, uint32_t *n_recv);
int mgx_halo_direct_connect_slots(mgx_world *w, uint32_t n_peers, const uint32_t *send_first, void *const *peer_recv_base,
                                  const uint64_t *peer_slot_capacity, const uint32_t *entry_slot, void *const *peer_flag_slot);
/* The exchange by hand: MGX_HALO_PUSH sends this rank's records for the next exchange,
 * MGX_HALO_WAIT fills the ghosts once every producer has done so; both = what the launches do by
 * themselves.  A launch that finds its exchange already pushed only waits — ranks that share one
 * process (and possibly a hardware queue) push all of them before the first one waits. */
#define MGX_HALO_PUSH 1u
#define MGX_HALO_WAIT 2u
int mgx_halo_direct_exchange(mgx_world *w, uint32_t what);
int mgx_halo_direct_status(mgx_world *w, uint64_t *exchanges, uint64_t *failed_exchange);
int mgx_halo_direct_disconnect(mgx_world *w);

/* ---- resident schedule launches on sharded worlds ----------------------------------------------------------------------
 * (replaces, like the exchanges above, the serial external phase and routing of robot.rs:1803-1859 and
 * factorgraph.rs:719-760 — here without ANY launch boundary or exchange kernel between the iterations of a schedule.)
 * A world whose robots all fit the device at once runs a whole mgx_iterate / mgx_tick schedule as ONE launch (one workgroup per
 * robot, resident for the schedule; neighbouring workgroups hand their snapshot records over inside the launch).  With the
 * calls below the same holds for a SHARDED world: every rank owns a GHOST AREA — fine-grained device memory holding, for each
 * ghost robot, its snapshot records and delivery counts for the two buffer parities and one progress word — which the ghosts'
 * owner ranks map (mgx_ipc_export / mgx_ipc_open across processes, raw pointers inside one process) and store into from
 * inside their own resident launch: a boundary robot's workgroup writes its records at the end of every segment into its own
 * rank's buffers AND (system-scope, over xGMI) into the ghost area of every rank that holds it as a ghost, then that ghost's
 * progress word; the workgroups there poll it like the word of a local neighbour.  One exchange per external iteration as
 * before (robot.rs:1803-1859), with no host work and no kernel boundary.  A schedule that OPENS with an external iteration
 * takes the direct exchange (above) in front of the launch, so mgx_halo_direct_* has to be connected too.
 *   1. mgx_halo_resident_setup (after mgx_halo_plan and mgx_halo_direct_setup_slots / _connect_slots): allocates the ghost area; returns its
 *      address, the number of ghost slots, this rank's buffer parity and segment count (both advance in lockstep on all ranks:
 *      every rank issues the same schedules), the slot of every entry of the receive list (recv_slots[n_recv]) and whether
 *      this rank CAN run resident launches (eligible: 1 — inter-robot factors staged in LDS, every local robot's workgroup
 *      resident at once; 2 — everything but inter-robot factors is there: on a world that follows its topology they may come
 *      later, and every schedule is decided where the ranks agree; 0 — no).  The ranks agree on that — all or none.
 *   2. mgx_halo_resident_connect_peers, ONCE: every peer's area (the peers of the direct exchange), its number of ghost slots,
 *      parity and segment count as returned by ITS setup (what translates this rank's counts into each peer's is settled here).
 *      coordinator_area / n_ranks: the area of rank 0 as this rank maps it (rank 0: its own) and the number of ranks of the
 *      world.  The first word of that area is where the ranks AGREE on every schedule: the launches of one schedule wait for
 *      each other's records, so they go ahead together or not at all.  Each rank's launch signs in there once all its own
 *      workgroups are on the device; the last rank to sign in says go; a rank that has waited MGX_RESIDENT_CENSUS_SHARDED_US
 *      (default 20000) for the others, or whose own workgroups do not all arrive (another tenant holds the CUs), or that cannot
 *      run this schedule as a resident launch at all, says abort — by system-scope compare-and-swap on that one word, so every
 *      rank reads the same answer before any of them has written anything.  After an abort every rank's world is as it was
 *      and the schedule runs launch by launch with the direct exchange (the engine does that by itself, see
 *      mgx_resident_outcome; the next few schedules skip the resident form — the same ones on every rank).
 *      coordinator_area NULL or n_ranks < 2: no agreement; a rank whose peers never start then gives up after
 *      MGX_RESIDENT_TIMEOUT_MS (default 2000) and reports MGX_ERR_STATE with the world invalid — never a hung GPU.
 *   3. mgx_halo_resident_aim, and again after every change of the lists, on every rank, with all ranks' launches through
 *      (synchronise, barrier): (local robot, index of the peer in connect_peers' order, the robot's ghost slot there) per
 *      boundary robot and peer that holds it as a ghost; the progress words of this rank's own ghosts start over at "through
 *      with everything so far" (a robot that has just become a neighbour across ranks never stored one here).
 * From then on mgx_iterate / mgx_tick run eligible schedules as one launch per rank (mgx_last_launch_count == 1); all ranks
 * must have connected.  A change of the world's layout (robots added / removed) switches the resident form off on THAT rank
 * only; the peers may still hold its area mapped and store into it, so wiring again goes: barrier, mgx_halo_resident_disconnect
 * on every rank, the peers close their mappings, barrier, then setup / connect_peers / aim as above.  A setup while the previous wiring
 * has not been disconnected is refused (MGX_ERR_STATE). */
int mgx_halo_resident_setup(mgx_world *w, void **area_base, uint32_t *n_ghost_slots, uint32_t *parity, uint64_t *segment_count,
                            int32_t *recv_slots, int32_t *eligible);
int mgx_halo_resident_connect_peers(mgx_world *w, uint32_t n_peers, void *const *peer_area_base, const uint32_t *peer_ghost_slots,
                                    const uint32_t *peer_parity, const uint64_t *peer_segment_count, void *coordinator_area, uint32_t n_ranks);
int mgx_halo_resident_aim(mgx_world *w, uint32_t n_targets, const int32_t *robots, const uint32_t *peer_index, const uint32_t *peer_slot);
int mgx_halo_resident_disconnect(mgx_world *w);
/* What became of the resident launch the last mgx_iterate enqueued (it decides within microseconds of its start whether it goes
 * ahead: residency census, and on sharded worlds the ranks' agreement above).  Waits for that decision.
 *   MGX_RESIDENT_NONE      nothing was pending (the call ran launch by launch, or its outcome has been taken already)
 *   MGX_RESIDENT_RAN       the launch goes ahead
 *   MGX_RESIDENT_DECLINED  the launch returned without touching the world, and the schedule has NOT been run: the caller
 *                          issues the same mgx_iterate again (it now takes the launch-by-launch path).
 * Nobody has to call this: every other entry point looks at the pending decision first and, after a declined launch, runs the
 * schedule launch by launch itself.  It exists for hosts that drive SEVERAL ranks from one thread (magics_amd/sharded.py:
 * LocalCluster): there the ranks' launch-by-launch exchanges must be enqueued in lockstep — all pushes before the first wait
 * — which a re-run inside one rank's call cannot do.  Only after mgx_iterate (a declined mgx_tick is re-run by the engine). */
#define MGX_RESIDENT_NONE 0
#define MGX_RESIDENT_RAN 1
#define MGX_RESIDENT_DECLINED 2
int mgx_resident_outcome(mgx_world *w, int32_t *outcome);
/* Whether mgx_iterate(w, steps, n) would be issued as a resident launch now — on a sharded world whose ranks agree on every
 * schedule (mgx_halo_resident_connect_peers): whether every rank takes it to that agreement (the same answer on every rank) — rather
 * than launch by launch.  For hosts that have to know in advance which form a schedule takes (LocalCluster, as above). */
int mgx_resident_ready(mgx_world *w, const uint8_t *steps, uint32_t n, int32_t *ready);
/* Resident launches of this world so far, how many of them were declined (see above; each is followed by a back-off during
 * which schedules skip the resident form), and what is left of the current back-off, in world-wide external iterations run
 * launch by launch (0: the next eligible schedule is tried as a resident launch).  Any pointer may be NULL. */
int mgx_resident_stats(mgx_world *w, uint64_t *launches, uint64_t *declined, uint32_t *backoff);
/* hipIpcGetMemHandle / hipIpcOpenMemHandle / hipIpcCloseMemHandle on the addresses above
 * (64-byte handles), so the host side needs no HIP binding of its own. */
int mgx_ipc_export(const void *dev_ptr, uint8_t handle[64]);
int mgx_ipc_open(const uint8_t handle[64], void **dev_ptr);
int mgx_ipc_close(void *dev_ptr);

/* ---- gbp_linalg + gbp_multivariate_normal value types (host only, no device) ---------------
 * crates/gbp_linalg/src/lib.rs:47-128: euclidean_norm = sqrt(fold(0, acc + x*x)), l1_norm,
 * normalize (untouched when the norm is 0 or infinite). */
double mgx_euclidean_norm(const double *x, uint32_t n);
double mgx_l1_norm(const double *x, uint32_t n);
void mgx_normalize(double *x, uint32_t n);
/* ndarray-inverse's contract as used by the reference (variable.rs:153,278; marginalise..:79;
 * gbp_multivariate_normal): det(); inverse = "None" (returns 0) exactly when det() == 0, else 1.
 * Row-major n x n. */
double mgx_det(const double *a, uint32_t n);
int mgx_inverse(const double *a, uint32_t n, double *out);

/* MultivariateNormal in information form (crates/gbp_multivariate_normal/src/lib.rs:38-410).
 * Errors mirror MultivariateNormalError (lib.rs:9-30); mgx_last_error() carries the variant text,
 * e.g. "VectorLengthNotEqualMatrixShape(3, 2, 2)". */
typedef struct mgx_mvn mgx_mvn;
#define MGX_MVN_ERR_NON_SQUARE (-16)          /* NonSquarePrecisionMatrix(rows, cols)            */
#define MGX_MVN_ERR_LENGTH (-17)              /* VectorLengthNotEqualMatrixShape(len, rows, cols) */
#define MGX_MVN_ERR_SINGULAR_PRECISION (-18)  /* NonInvertiblePrecisionMatrix                     */
#define MGX_MVN_ERR_SINGULAR_COVARIANCE (-19) /* NonInvertibleCovarianceMatrix                    */
#define MGX_MVN_ADD 0
#define MGX_MVN_SUB 1
#define MGX_MVN_MUL 2 /* product of densities = sum in information form (lib.rs:380-410) */
/* lib.rs:63-93: checks in this order: square, lengths, det == 0; mean = precision . information */
int mgx_mvn_from_information_and_precision(const double *information, uint32_t len,
                                           const double *precision, uint32_t rows, uint32_t cols,
                                           mgx_mvn **out);
/* lib.rs:114-143 */
int mgx_mvn_from_mean_and_covariance(const double *mean, uint32_t len, const double *covariance,
                                     uint32_t rows, uint32_t cols, mgx_mvn **out);
void mgx_mvn_destroy(mgx_mvn *m);
uint32_t mgx_mvn_len(const mgx_mvn *m);
/* information_vector(), precision_matrix(), mean() (any pointer may be NULL); covariance() */
int mgx_mvn_get(const mgx_mvn *m, double *information, double *precision, double *mean);
int mgx_mvn_covariance(const mgx_mvn *m, double *covariance);
/* update_information_vector / update_precision_matrix (lib.rs:158-178); set_* and add_assign_*
 * (the `unsafe` ones, lib.rs:212-263: mean stale until update); update() returns 1 if the mean
 * was recomputed, 0 if it was current (lib.rs:271-279) */
int mgx_mvn_update_information_vector(mgx_mvn *m, const double *value);
int mgx_mvn_update_precision_matrix(mgx_mvn *m, const double *value);
int mgx_mvn_set_information_vector(mgx_mvn *m, const double *value);
int mgx_mvn_set_precision_matrix(mgx_mvn *m, const double *value);
int mgx_mvn_add_assign_information_vector(mgx_mvn *m, const double *value);
int mgx_mvn_add_assign_precision_matrix(mgx_mvn *m, const double *value);
int mgx_mvn_update(mgx_mvn *m);
/* a op b -> new value (Add / Sub / Mul, lib.rs:300-410) and a op= b */
int mgx_mvn_combine(const mgx_mvn *a, const mgx_mvn *b, int32_t op, mgx_mvn **out);
int mgx_mvn_combine_assign(mgx_mvn *a, const mgx_mvn *b, int32_t op);

/* ---- environment rasteriser (scenario front-end) --------------------------- */
/* gbp_environment::Environment (crates/gbp_environment/src/lib.rs:729-735) as plain data, and
 * env_to_png::env_to_image / env_to_sdf_image (crates/env_to_png/src/lib.rs:149-206) computed on
 * the device: what simulation_loader.rs:154-162 runs for each scenario to produce the image the
 * obstacle factors sample.  Images are interleaved RGB u8 (R = G = B), row-major,
 * (n_cols * resolution) x (n_rows * resolution).  Invalid input (a value the reference's
 * Percentage / StrictlyPositiveFinite / Angle / RelativePoint constructors reject, an empty grid)
 * returns MGX_ERR_INVALID where the reference panics or returns Err. */
#define MGX_SHAPE_CIRCLE 0          /* radius                         (lib.rs:114-143) */
#define MGX_SHAPE_TRIANGLE 1        /* angle_a, angle_b, radius       (lib.rs:158-223) */
#define MGX_SHAPE_REGULAR_POLYGON 2 /* sides, radius                  (lib.rs:232-300) */
#define MGX_SHAPE_POLYGON 3         /* n_points, points_xy            (lib.rs:345-415) */
#define MGX_SHAPE_RECTANGLE 4       /* width, height                  (lib.rs:305-340) */
typedef struct mgx_env_obstacle { /* gbp_environment::Obstacle (lib.rs:531-543) */
    int32_t shape;                /* MGX_SHAPE_*                                              */
    int32_t tile_row, tile_col;   /* tile_coordinates                                         */
    uint32_t sides;               /* regular polygon                                          */
    uint32_t n_points;            /* polygon                                                  */
    const double *points_xy;      /* polygon: n_points (x, y) pairs, each in [0, 1]           */
    double radius;                /* circle, triangle (inscribed circle), regular polygon     */
    double angle_a, angle_b;      /* triangle: Angles { A, B } in radians                     */
    double width, height;         /* rectangle                                                */
    double rotation;              /* radians in [0, 2 pi] (angle::Angle)                      */
    double translation_x, translation_y; /* RelativePoint: each in [0, 1]                     */
} mgx_env_obstacle;
typedef struct mgx_env_desc {
    uint32_t n_rows, n_cols;      /* TileGrid::shape (lib.rs:45-63)                           */
    const uint32_t *tiles;        /* n_rows * n_cols Unicode scalar values, row-major         */
    float tile_size, path_width;  /* TileSettings (lib.rs:589-597)                            */
    uint32_t sdf_resolution;      /* SdfSettings (lib.rs:599-617): pixels per tile,           */
    float sdf_expansion, sdf_blur; /*   expansion and blur as fractions of a tile             */
    uint32_t n_obstacles;
    const mgx_env_obstacle *obstacles;
} mgx_env_desc;
int mgx_env_image_size(const mgx_env_desc *env, uint32_t resolution, uint32_t *width, uint32_t *height);
/* env_to_image(env, resolution, expansion) (env_to_png lib.rs:165-206) */
int mgx_env_to_image(const mgx_env_desc *env, uint32_t resolution, float expansion, uint8_t *rgb);
/* env_to_sdf_image(env, resolution, expansion, blur_percent) (lib.rs:149-163): the image above,
 * blurred with image::imageops::blur(sigma = blur_percent * resolution) unless sigma < 1 */
int mgx_env_to_sdf_image(const mgx_env_desc *env, uint32_t resolution, float expansion,
                         float blur_percent, uint8_t *rgb);
/* The call chain of simulation_loader.rs:154-162 + robot.rs:1259-1264: rasterise with the
 * environment's own sdf settings and install the result as the world's obstacle image, world
 * size = tile_size * (n_cols, n_rows). */
int mgx_world_set_environment(mgx_world *w, const mgx_env_desc *env);

/* ---- robot-environment collisions: the map's colliders and the pass on the device ---------------------------
 * update_robot_environment_collisions (planner/collisions.rs:368-438): every robot's Ball against every Collider that
 * build_tile_grid piped into build_obstacles produced (environment/map_generator.rs:141-514, 537-1293), through the same
 * Free / Colliding state machine as robot pairs (collisions.rs:455-493); export.rs:190-220, 379, 553 writes the count per
 * robot and the contacts per (robot, obstacle).
 *
 * mgx_env_colliders (host code, no device needed): the colliders in the reference's creation order — the tile cuboids row by
 *   row, tile by tile, in the order of each tile's vec![..], then the placeable obstacles in list order.  The index in that
 *   order is the collider's identity everywhere below (it stands in for the reference's mesh Entity).  Everything is computed
 *   in f32 as map_generator.rs writes it (base_dim, pos_offset with its mul_add, the grid offsets), quirks included: the
 *   circle's z uses 1 - y and is not negated and its radius is radius * tile_size; the rectangle has w * tile_size / 4,
 *   h * tile_size / 4 half extents and no rotation; the triangle's points are mirrored in x, rotated by
 *   Quat::from_rotation_y(pi/2 - rot) and placed under an isometry of angle -rot on top of that; the regular polygon's points
 *   are rotated by rot + rotation_offset, scaled by tile_size / 2 and placed under an isometry of the same angle again; the
 *   polygon's points are scaled by tile_size and not rotated.  A Bevy Cuboid::new(x, y, z) becomes a 2-D cuboid of half
 *   extents (x / 2, z / 2) at (translation.x, translation.z) (the conversion lives in the reference's parry fork;
 *   tests/test_env_colliders.py pins this reading against the rasteriser).  ConvexPolygon::from_convex_hull and
 *   Triangle::new become a convex hull computed here (monotone chain: counter-clockwise, collinear points dropped), stored as
 *   WORLD-space vertices (isometry applied); mins / maxs of a polygon are the bounds of those vertices.
 *   out [capacity], vertices_xz [vertex_capacity][2]: filled as far as they reach; *n / *n_vertices: the full counts (NULL
 *   outputs with capacity 0 return the counts; MGX_ERR_INVALID if a non-zero capacity is too small).  An environment the
 *   rasteriser rejects at any resolution and expansion (empty grid, a value the reference's Percentage /
 *   StrictlyPositiveFinite / Angle / RelativePoint constructors reject, an unknown shape: one shared validation) returns
 *   MGX_ERR_INVALID.
 *
 * SPECIFICATION OF A CONTACT.  This is the specification, not a claim about parry2d: its query::intersection_test (GJK for
 *   the polygons) is third party and absent from the reference's tree, so there is nothing to be bit-identical to; the two
 *   can differ only for centres within rounding of tangency, which nothing available pins.
 *   A robot is (x, z) = Transform (x, z) and r = (float)desc.radius, alive as the robot-robot pass defines alive.  It touches
 *   a collider iff the distance from its centre to the closed shape is <= r, in f32 with every operation rounded on its own
 *   (the same in libmgx.so and libmgx_fma.so):
 *     ball      dx*dx + dz*dz <= (r + R)*(r + R), d = p - t;
 *     cuboid    (no rotation) e = max(|p - t| - h, 0) per axis, e_x*e_x + e_z*e_z <= r*r;
 *     polygon   (world vertices v_0 .. v_{n-1}, counter-clockwise; edge i from a = v_i to b = v_{(i+1) % n}, e = b - a,
 *               q = p - a) the centre is inside (e_x*q_z - e_z*q_x >= 0 for every edge, and r == r), or the smallest over the
 *               edges of |q - t e|^2, t = min(max((q_x*e_x + q_z*e_z) / (e_x*e_x + e_z*e_z), 0), 1) (t = 0 for an edge of
 *               length 0), is <= r*r;
 *     a NaN anywhere means no contact.
 *   A contact that was not one after the pass before (or was not looked at: the robot was not alive, or is new) is one
 *   EVENT {pass, robot, collider, mins, maxs}: mins = max(p - r, collider.mins), maxs = min(p + r, collider.maxs) per axis
 *   (robot_aabb intersected with Collider::aabb(), collisions.rs:417-426), and counts once for the robot.  A robot that is
 *   not alive or has a non-finite coordinate is Free of everything.
 *
 * mgx_env_collisions_enable(w, env, event_capacity): builds the collider table of `env` and uploads it once, together with a
 *   uniform grid over the world (a cell is one tile; per cell the colliders whose AABB overlaps it, built on the host: the
 *   map is static).  event_capacity (0: 262144) records of log are allocated here and never grow.  env == NULL switches off
 *   and drops the state.  Default: off — no kernel, no allocation, no change to anything else.  Calling it while on is
 *   MGX_ERR_STATE (switch off first).
 * While on, every mgx_mission_tick_end (so every mgx_mission_tick and every tick of mgx_mission_run) enqueues one pass on the
 *   Transforms after that tick's move and the robots alive after that tick's despawns, beside the robot-robot pass: no
 *   synchronisation, nothing read back.
 * mgx_env_collisions_update: the same pass over positions the caller keeps ([n_robots][3], x and z are read; NULL: the
 *   device's mission Transforms as they are).  Enqueued, not waited for.
 * mgx_env_collisions_read: the one call that synchronises.  events [first, first + capacity) of the log in (pass, robot,
 *   collider) order, *n_total = events in the log, *dropped = events that found the log full (counted, not stored; the
 *   per-robot counts include them), per_robot [n_robots] (may be NULL).  The device remembers up to 8 colliders a robot
 *   touches at the same time; if a robot ever touched more, the call fills its outputs and returns MGX_ERR_STATE (contacts
 *   beyond the eighth may have been logged again).
 * mgx_env_collisions_clear: everybody Free, log and counts empty, pass 0.
 * Unsharded worlds (MGX_ERR_STATE on a world with ghosts); MGX_ERR_STATE from _update / _read / _clear while switched off. */
#define MGX_COLLIDER_BALL 0
#define MGX_COLLIDER_CUBOID 1
#define MGX_COLLIDER_POLYGON 2
typedef struct mgx_env_collider {
    int32_t kind;                 /* MGX_COLLIDER_BALL / _CUBOID / _POLYGON (triangles and hulls)            */
    int32_t tile_row, tile_col;   /* the tile it came from                                                   */
    int32_t obstacle;             /* index into env->obstacles, -1 for a tile-grid cuboid                    */
    float   tx, tz, angle;        /* the Isometry2 the reference builds                                      */
    float   radius;               /* ball                                                                    */
    float   half_extents[2];      /* cuboid                                                                  */
    uint32_t first_vertex, n_vertices; /* polygon: WORLD-space vertices (isometry applied), counter-clockwise */
    float   mins[2], maxs[2];     /* Collider::aabb() in world (x, z)                                        */
} mgx_env_collider;
int mgx_env_colliders(const mgx_env_desc *env, mgx_env_collider *out, uint32_t capacity, uint32_t *n,
                      float *vertices_xz, uint32_t vertex_capacity, uint32_t *n_vertices);
typedef struct mgx_env_collision_event {
    uint64_t pass;
    int32_t robot, collider;
    float mins[2], maxs[2];       /* (x, z) */
} mgx_env_collision_event;
int mgx_env_collisions_enable(mgx_world *w, const mgx_env_desc *env, uint64_t event_capacity);
int mgx_env_collisions_update(mgx_world *w, const float *positions_xyz);
int mgx_env_collisions_read(mgx_world *w, uint64_t first, mgx_env_collision_event *events, uint64_t capacity,
                            uint64_t *n_total, uint64_t *dropped, uint32_t *per_robot);
int mgx_env_collisions_clear(mgx_world *w);

/* ---- goal areas on the device: the first arrival of every robot in every area ----------------------------------
 * goal_area::detect_collisions (crates/magics/src/goal_area.rs:67-103, FixedUpdate): every robot carries a
 * goal_area::components::Collider(Ball::new(radius)) (planner/spawner.rs:638); per goal area the reference records the first
 * time each robot's ball intersects the area's box, and export.rs:235-247, 261, 556-571 writes it as
 * goal_areas: {area: {aabb, history: {robot: seconds}}}, which scripts/analyse-junction-scenario.py:52-109 reads (the
 * throughput of a junction).  The one system that spawns areas (setup_goal_areas_for_junction_scenario, goal_area.rs:105-119)
 * is commented out of the reference's plugin, so its exports carry an empty map; here the caller hands the areas in.
 * Restated on the host by magics_amd/sim.py (goal_area_contacts, _goal_areas_host), which is the checker.
 * AREA: mgx_goal_area {mins, maxs} in world (x, z), the plane the collision passes use.  The corners are sorted per axis when
 *   the areas are set (mins = min of the two, maxs = max): the reference's first junction area is written with its second
 *   coordinates swapped, Aabb::new((-8, -48), (8, -52)).  Centre c = (mins + maxs) * 0.5f and half extents
 *   h = (maxs - mins) * 0.5f, in f32, every operation rounded on its own.  At most MGX_GOAL_AREAS_MAX areas.
 * CONTACT: the cuboid line of the SPECIFICATION OF A CONTACT above with t = c, h as here and r = (float)desc.radius:
 *   e = max(|p - c| - h, 0) per axis, e_x*e_x + e_z*e_z <= r*r, in f32, nothing contracted (the same in libmgx.so and
 *   libmgx_fma.so; the device runs the very predicate of the robot-environment pass); a NaN anywhere means no contact.  As
 *   there, this is the specification, not a claim about parry2d.
 * WHO: the robots alive as the robot-robot pass defines alive (not removed, not ghosts) — idle robots and robots whose mission
 *   is complete included: they are still in the reference's query.
 * STATE per (area, robot id): the tick of the first pass in which the two touched, or "never".  Once set it never changes
 *   (history.contains_key -> continue); the arrivals of robots despawned later stay.  The table is no part of the blob layout:
 *   it survives an in-place append, a relayout, and a robot that joins between mgx_mission_tick_begin and _end, as the
 *   trackers' arrays do; robots added later start at "never".  On a world with head-room (mgx_world_reserve) the table is
 *   strided for the reserved robots, so an append does not move it.
 * CLOCK: one u64 per world, the index k of the coming tick — a clock of its own (the trackers may be off).  The device stores
 *   tick indices only (k + 1 in 32 bits: a tick beyond 2^32 - 2 is MGX_ERR_INVALID).  Seconds are made on the host:
 *   elapsed = (k + 1) * tick_ns as a duration of whole seconds and nanoseconds, value = (float)secs + (float)nanos / 1e9f —
 *   Duration::as_secs_f32, which Time<Fixed>::elapsed_seconds() returns inside the k-th FixedUpdate.  bevy_time is third party
 *   and absent from the reference's tree: this reading is the specification.
 * mgx_goal_areas_enable(w, areas, n_areas, next_tick): on (default: off — no kernel, no allocation, no change to anything
 *   else).  n_areas == 0 switches off and drops the state.  Calling it while on is MGX_ERR_STATE (switch off first).
 *   MGX_ERR_INVALID: a non-finite corner, more than MGX_GOAL_AREAS_MAX areas, areas == NULL with n_areas > 0.
 * mgx_goal_areas_set_clock: the tick index of the coming tick.
 * While on, every mgx_mission_tick_end (so every mgx_mission_tick and every tick of mgx_mission_run) enqueues ONE pass on the
 *   Transforms after that tick's move and the robots alive after that tick's despawns, beside the collision passes; the clock
 *   then advances by one.  No synchronisation, nothing read back; no launch while no robot is alive.
 * mgx_goal_areas_update: the same pass over positions the caller keeps ([n_robots][3], x and z are read; NULL: the device's
 *   mission Transforms as they are), at a tick the caller names.  Does not move the clock; enqueued, not waited for.
 * mgx_goal_areas_read: the one call that synchronises.  Every arrival in (tick, robot, area) order; *n_total and per_area
 *   [n_areas] (may be NULL) are always filled.  capacity 0 asks for the size; a non-zero capacity below *n_total is
 *   MGX_ERR_INVALID.
 * mgx_goal_areas_clear: everybody "never"; the areas and the clock stay.
 * Unsharded worlds (MGX_ERR_STATE on a world with ghosts); MGX_ERR_STATE from every call but _enable while switched off. */
#define MGX_GOAL_AREAS_MAX 64u
typedef struct mgx_goal_area {      /* 16 bytes */
    float mins[2], maxs[2];         /* (x, z); either order per axis */
} mgx_goal_area;
typedef struct mgx_goal_arrival {   /* 16 bytes */
    uint64_t tick;
    int32_t area, robot;
} mgx_goal_arrival;
int mgx_goal_areas_enable(mgx_world *w, const mgx_goal_area *areas, uint32_t n_areas, uint64_t next_tick);
int mgx_goal_areas_set_clock(mgx_world *w, uint64_t next_tick);
int mgx_goal_areas_update(mgx_world *w, const float *positions_xyz, uint64_t tick);
int mgx_goal_areas_read(mgx_world *w, mgx_goal_arrival *arrivals, uint64_t capacity, uint64_t *n_total,
                        uint32_t *per_area /* [n_areas] or NULL */);
int mgx_goal_areas_clear(mgx_world *w);

/* ---- trackers on the device: position and velocity samples, distance travelled ---------------------------------
 * track_positions / track_velocities (crates/magics/src/planner/tracking.rs:117-136, 210-240; both on 100 ms timers,
 * planner/spawner.rs:627-628) and the distance travelled the export carries (export.rs:249-262), restated on the host by
 * magics_amd/sim.py (_track / _tracks) and magics_amd/driver.py (Driver.tick), which are the checkers.
 * STATE per robot id (ids are stable and never reused): elapsed_ns (0), a has-previous flag with the previous sample's position
 *   (f32[3]) and tick, travelled (f64, 0).  Robots added after _enable start from zero state, the others keep theirs — through an
 *   in-place append, a relayout, or a join between mgx_mission_tick_begin and _end: the arrays are no part of the blob layout.
 * CLOCK: one u64 per world, the simulated tick index k of the coming tick; the time of tick k is
 *   t(k) = (double)((k + 1) * tick_ns) * 1e-9 — the integer product is exact, there is ONE f64 multiplication.
 * A PASS takes a tick k, positions [n][3] as f32 and a "moved this tick" byte per robot.  For every robot that moved:
 *   elapsed_ns += tick_ns; if elapsed_ns < period_ns nothing else happens, otherwise elapsed_ns %= period_ns and ONE sample is
 *   taken (at most one per tick): {tick = k, robot, position = p, span_ticks = k - previous tick (0: the robot's first sample)}
 *   and, when span_ticks != 0, velocity[c] = (p[c] - prev[c]) / (float)(t(k) - t(k - span_ticks)), c = 0..2: the difference of
 *   the times in f64, rounded to f32 once; the subtraction and the division each rounded to f32 on their own, the division
 *   correctly rounded, nothing contracted — libmgx.so and libmgx_fma.so agree bit for bit.  Then prev = (p, k), also when the
 *   log is full, so that later velocities stay right.  Robots that did not move keep their timers: idle, completed and removed
 *   robots take no sample.
 * DISTANCE is accumulated in the mission chain only, every tick, for every robot that moves, whatever its timer says:
 *   c0 = ts * (mu_x[1] - mu_x[0]), c1 likewise for y — the values k_mission_prepare casts into the Transform (robot.rs:2314) —
 *   travelled += sqrt(c0*c0 + c1*c1), every operation rounded to f64 on its own, no FMA in either library.
 * LOG: append-only in device memory, sample_capacity records allocated by _enable (0: 262144), never growing.  A sample that
 *   finds the log full is counted in `dropped`, not stored; which samples of the overflowing tick are kept is unspecified.
 * mgx_tracks_enable(w, 1, period_ns, tick_ns, next_tick, sample_capacity): on (default: off — no kernel, no allocation);
 *   period_ns and tick_ns > 0.  While on, every mgx_mission_tick_end (so every mgx_mission_tick and every tick of
 *   mgx_mission_run) enqueues ONE pass on the world's stream over the Transforms after that tick's move, with "moved" = the
 *   robots the tick moves, behind the Transform increment and in front of the prior updates; the clock then advances by one.
 *   No synchronisation, nothing read back.  Enabling again while on keeps everything and sets the clock (other timers or
 *   another capacity: MGX_ERR_STATE).  enabled = 0 drops the state.
 * mgx_tracks_set_clock: the tick index of the coming tick.
 * mgx_tracks_update: the same sampling pass over positions the caller keeps, at a tick the caller names (positions_xyz NULL: the
 *   device's mission Transforms; moved NULL: every live robot; a removed robot never moves).  Adds no distance, does not move
 *   the clock; enqueued, not waited for.
 * mgx_tracks_take: the one call that synchronises.  *n_in_log and *dropped are always filled, travelled [n_robots] if given.  If
 *   capacity >= *n_in_log the whole log is copied out in (tick, robot) order and emptied (*n_taken = *n_in_log; per-robot
 *   state, distances and `dropped` stay); otherwise nothing is taken and *n_taken = 0 — capacity 0 asks for the size.
 * mgx_tracks_clear: the log empty, `dropped` and the distances zero, every robot's timer and previous sample forgotten.
 * Unsharded worlds (MGX_ERR_STATE on a world with ghosts); MGX_ERR_STATE from every other call while switched off. */
typedef struct mgx_track_sample {   /* 40 bytes */
    uint64_t tick;
    int32_t  robot;
    uint32_t span_ticks;            /* 0: first sample of this robot, velocity not set (zeros) */
    float    position[3], velocity[3];
} mgx_track_sample;
int mgx_tracks_enable(mgx_world *w, int32_t enabled, uint64_t period_ns, uint64_t tick_ns, uint64_t next_tick, uint64_t sample_capacity);
int mgx_tracks_set_clock(mgx_world *w, uint64_t next_tick);
int mgx_tracks_update(mgx_world *w, const float *positions_xyz, const uint8_t *moved, uint64_t tick);
int mgx_tracks_take(mgx_world *w, mgx_track_sample *samples, uint64_t capacity, uint64_t *n_taken, uint64_t *n_in_log,
                    uint64_t *dropped, double *travelled /* [n_robots] or NULL */);
int mgx_tracks_clear(mgx_world *w);

/* ---- run metrics on the device: dimensionless jerk and path deviation per robot ----------------------------------
 * What the reference's analysis scripts compute from an export — smoothness (scripts/ldj.py:17-55, Log Dimensionless Jerk) and
 * perpendicular path deviation (scripts/perpendicular-path-deviation.py:40-60, 99-115) — carried as O(1) state per robot and
 * updated by the tracker pass at the moment a sample is taken, so that a run needs no sample log.  Restated on the host by
 * magics_amd/track_metrics.py, the checker.  The lane arithmetic: magics_amd/csrc/mgx_track_metrics.h.
 * ARITHMETIC: f64, every operation rounded on its own, nothing contracted, division and square root correctly rounded:
 *   libmgx.so and libmgx_fma.so agree bit for bit.  sq2(a, b) = (a*a) + (b*b).  There is no logarithm on the device: it
 *   reports the dimensionless jerk DJ, and LDJ = -log(DJ) is the caller's.
 * VELOCITY SERIES of a robot: u_i = (double)velocity[0], w_i = (double)velocity[2] of its samples with span_ticks != 0, in the
 *   order they are made, i = 0 .. n-1 (the reference's columns [0, 2], ldj.py:92).
 * JERK, free of times.  g(x)_0 = x_1 - x_0, g(x)_{n-1} = x_{n-1} - x_{n-2}, g(x)_i = (x_{i+1} - x_{i-1}) / 2 otherwise
 *   (np.gradient with unit spacing); a = g(x), j = g(a), where a difference of two a's is formed it is (later - earlier);
 *   q_i = sq2(g(g(u))_i, g(g(w))_i); W = the composite Simpson sum of q with unit spacing under scipy.integrate.simpson's rule
 *   (scipy >= 1.11): n odd: (q_0 + 4 O + 2 E + q_{n-1}) / 3 with O the sum over odd i and E over even interior i; n even: the
 *   same over q_0 .. q_{n-2}, plus (5/12) q_{n-1} + (2/3) q_{n-2} - (1/12) q_{n-3}.  vmax2 = max_i sq2(u_i, w_i).
 *   DJ = (n-1)^3 W / vmax2.  This is ldj.py's figure: it differentiates with dt = the mean spacing of the time stamps and
 *   integrates over linspace(t_0, t_{n-1}, n), whose spacing is the same dt; with T = (n-1) dt,
 *   T^3 / vmax^2 * (dt * W / dt^4) = (n-1)^3 W / vmax2.  Valid for n >= 3 and vmax2 > 0; otherwise DJ = NaN and the flag is
 *   clear (the reference asserts or divides by zero there).
 * STREAMING, and the ORDER OF THE SUMS.  State: n, the last five velocities, q0, s_odd, s_even, hold, vmax2 (all zero at first).
 *   When velocity m = n arrives: it enters the window; vmax2 = max(vmax2, sq2(u, w)); n = m + 1; then
 *     m == 3: q0 = q_0 and s_odd = q_1 (both final from here on: a_0 one-sided, a_1 and a_2 central);
 *     m >= 4: q = q_{m-2}, from a_{m-1} = (x_m - x_{m-2}) / 2 and a_{m-3} = (x_{m-2} - x_{m-4}) / 2, j = (a_{m-1} - a_{m-3}) / 2;
 *             if m >= 5 the value held so far, q_{m-3}, is added to s_odd (m-3 odd) or s_even (m-3 even); then hold = q.
 *   So s_odd = ((q_1 + q_3) + q_5) + ..., s_even = ((0 + q_2) + q_4) + ... up to index n-4, and hold = q_{n-3}: arrival order.
 *   FINALISATION works on a copy of the state whenever somebody reads; the accumulation goes on undisturbed.  With
 *   a_{n-1} = x_{n-1} - x_{n-2}:
 *     n == 3: a_0 = x_1 - x_0, a_1 = (x_2 - x_0) / 2; q_0 = sq2(a_1 - a_0), q_1 = sq2((a_2 - a_0) / 2), q_2 = sq2(a_2 - a_1);
 *             W = ((q_0 + 4 q_1) + q_2) / 3.
 *     n >= 4: a_{n-2} = (x_{n-1} - x_{n-3}) / 2, a_{n-3} = (x_{n-2} - x_{n-4}) / 2, qa = q_{n-2} = sq2((a_{n-1} - a_{n-3}) / 2),
 *             qb = q_{n-1} = sq2(a_{n-1} - a_{n-2});
 *       n odd:  O = s_odd + qa, E = s_even + hold, W = (((q0 + 4 O) + 2 E) + qb) / 3;
 *       n even: O = s_odd + hold and qc = hold (n == 4: O = qc = s_odd), W = (((q0 + 4 O) + 2 s_even) + qa) / 3
 *               + (((5/12) qb + (2/3) qa) - (1/12) qc), the three constants being the f64 quotients.
 *     T = (double)(n - 1), DJ = (((T T) T) W) / vmax2.
 * PATH DEVIATION.  For every sample taken, first samples included: p = ((double)position[0], (double)position[2]).  Over the
 *   segments (a, b) of the robot's route polyline, in order, with d = b - a and l2 = sq2(d_x, d_y) > 0:
 *   dist = |d_x (p_y - a_y) - d_y (p_x - a_x)| / sqrt(l2) (each product rounded, then the difference); the sample's deviation is
 *   the smallest (the first on ties); deviation_sum += deviation, deviation_max = max(deviation_max, deviation),
 *   n_positions += 1.  This is the reference's distance to the INFINITE lines through consecutive waypoints.  The difference:
 *   its slope-intercept form yields inf / NaN for a vertical segment or one of zero length; here a vertical segment is a line
 *   like any other and a segment of zero length is left out.  Elsewhere the two agree up to rounding.  A sample taken while
 *   the robot has no route, or none with a segment of non-zero length, is counted in n_unrouted and not in n_positions.  The
 *   reference's "RMSE" is sqrt(deviation_sum / n_positions) (sic, :114-115).
 * mgx_track_metrics_enable(w, 1, max_route_points): on (default: off — no allocation, no extra work in the pass).  Needs the
 *   trackers on (MGX_ERR_STATE otherwise, and on a world with ghosts); max_route_points in 2 .. 65536, 0: 16.  Enabling again
 *   while on keeps everything (another max_route_points: MGX_ERR_STATE).  The state follows the tracker state's rules: robots
 *   added later start from zero and without a route, and the state survives an in-place append, a relayout and a join between
 *   mgx_mission_tick_begin and _end.  mgx_tracks_clear zeroes it (routes stay), mgx_tracks_enable(.. 0 ..) drops it, and so
 *   does enabled = 0 here.
 * mgx_track_metrics_set_route(w, robot, xy, n_points): the polyline [n_points][2] (x, z of the world) the deviation is measured
 *   against, uploaded in stream order: it holds for the samples of passes enqueued after the call.  n_points = 0 clears it;
 *   more than max_route_points: MGX_ERR_INVALID.  It can be replaced at any time.
 * mgx_tracks_set_logging(w, on): default on (and on again after mgx_tracks_enable(.. 0 ..)).  Off: a sample still moves the
 *   timer, the previous sample, the distance and the metrics, but is not appended: the cursor does not move and `dropped`
 *   does not count.
 * mgx_track_metrics_read(w, out, capacity): the one call that synchronises; finalises every robot on a copy into
 *   out[0 .. n_robots) (capacity < n_robots: MGX_ERR_INVALID).  flags: MGX_TRACK_JERK_VALID, MGX_TRACK_DEVIATION_VALID
 *   (n_positions > 0). */
#define MGX_TRACK_JERK_VALID      1u
#define MGX_TRACK_DEVIATION_VALID 2u
typedef struct mgx_track_metrics {  /* 48 bytes */
    uint32_t n_positions, n_velocities, n_unrouted, flags;
    double   dimensionless_jerk;    /* NaN unless MGX_TRACK_JERK_VALID */
    double   vmax2, deviation_sum, deviation_max;
} mgx_track_metrics;
int mgx_track_metrics_enable(mgx_world *w, int32_t enabled, uint32_t max_route_points);
int mgx_track_metrics_set_route(mgx_world *w, int32_t robot, const double *xy, uint32_t n_points);
int mgx_tracks_set_logging(mgx_world *w, int32_t on);
int mgx_track_metrics_read(mgx_world *w, mgx_track_metrics *out, uint64_t capacity);

/* ---- global planner: batched RRT* over the map's colliders -------------------------------------------------------
 * What crates/gbp_global_planner does for one robot (rrtstar.rs:15-83; started from progress_missions, robot.rs:578-633),
 * for many requests in one call: a formation spawns and every robot of it asks at once.  The paths it returns are what
 * mgx_apply_global_paths takes.
 *
 * SPECIFICATION OF A PLAN.  This is the specification, not a claim about the `rrt` crate: the reference calls a git fork of it
 *   (Cargo.toml:72-84) that is absent from its tree, as is `rand`, so there is nothing to be bit-identical to.
 *   magics_amd/global_planner.py restates it on the host and is the checker of the device.
 *   ARITHMETIC.  f64, every operation rounded on its own (the same in libmgx.so and libmgx_fma.so): d2(a, b) = dx*dx + dy*dy,
 *     dist = sqrt(d2).  Planner (x, y) is the collider table's (x, z), the frame of the contact specification above: no flip.
 *   feasible(p): no collider of the table touches a ball at ((float)p.x, (float)p.y) with radius collision_radius under the
 *     specification of a contact above.  Points outside the grid are feasible unless a collider reaches them.  Neither the root
 *     nor `end` is tested (the reference hands only tree nodes to its callback).
 *   RANDOM STREAM.  One wyrand state per request (state += 0xA0761D6478BD642F; t = state * (state ^ 0xE7037ED1A0B428DB) in 128
 *     bits; next_u64 = hi(t) ^ lo(t); next_u32 = its low half).  uniform(h): u = next_u64,
 *     v = f64_from_bits((u >> 12) | 0x3FF0000000000000) - 1.0, result v*(2h) + (-h).  A sample is (uniform(h), uniform(h)), x
 *     first, h = sample_half_extent.  gen_index(n) is rand 0.8.5's UniformInt::<u32>::sample_single(0, n): zone =
 *     (n << clz(n)) - 1; draw next_u32 until lo32(draw * n) <= zone; the result is hi32(draw * n).
 *   TREE GROWTH.  Node 0 is ((double)start.x, (double)start.y), cost 0, no parent.  Iteration i = 1 .. max_iterations:
 *     1. q = sample.
 *     2. n* = the node with the smallest d2(node, q); ties: the lowest index.
 *     3. d = sqrt(d2*).  d == 0: the iteration ends.  d <= step: p = q.  Otherwise t = step / d, p = n* + t*(q - n*) per axis.
 *     4. !feasible(p): the iteration ends.
 *     5. N = the nodes with d2(node, p) <= radius*radius.
 *     6. parent = the k in N u {n*} with the smallest cost[k] + dist(k, p); ties: the lowest index.  That value is cost_new.
 *     7. The tree already holds max_nodes: the request ends with MGX_PLAN_TREE_FULL.  Otherwise append m = (p, parent, cost_new).
 *     8. Rewire: for k in N, k != parent: c = cost_new + dist(k, p); c < cost[k]: parent[k] = m, cost[k] = c.  Descendants'
 *        costs are NOT propagated.
 *     9. dist(p, end) <= step: the goal is reached at m, growth stops (the first reach), and the path's cost is
 *        cost_new + dist(p, end).
 *     max_iterations without a reach: MGX_PLAN_MAX_ITERATIONS (PathfindingError::ReachedMaxIterations).
 *   PATH.  The parent chain from m to node 0, reversed, then `end`.
 *   SMOOTHING.  If enabled, while the path has >= 3 points, for s < smoothing_max_iterations: a = gen_index(len - 2);
 *     b = a + 2 + gen_index(len - 2 - a); L = dist(P[a], P[b]); the chord is free iff feasible(P[a] + (P[b] - P[a]) * ((j*h)/L))
 *     for every j = 1 .. floor(L/h), h = smoothing_step; a free chord deletes P[a+1 .. b-1].
 *   Points go out as f32.  A request that fails has no points.
 *
 * mgx_planner_enable(w, env, params): builds the collider table of `env` and uploads it with the per-tile grid the
 *   robot-environment pass uses (its own copy: either can be switched off without the other).  env == NULL switches off and drops
 *   every allocation.  Default: off — no allocation, no change to anything else.  Calling it while on replaces map and
 *   parameters.  MGX_ERR_INVALID: step_size, neighbourhood_radius (and smoothing_step when smoothing is enabled) not positive
 *   and finite, collision_radius or sample_half_extent negative or not finite, max_nodes beyond 65536.  The positions of a
 *   tree live in the workgroup's LDS: max_nodes beyond 8192 needs more of it than a gfx950 CU has and fails at the launch.
 * mgx_plan_paths(w, n, requests, results, path_xy, point_capacity, n_points): plans the n requests, synchronously (like every
 *   other call it first ends a lingering launch).  One workgroup per request; a launch runs at most iterations_per_launch
 *   iterations of every request (growth and smoothing iterations alike) and the host launches again until every request has
 *   ended: no kernel is unbounded, and the result does not depend on where the slices fall.  The call is the pool of PLANS THAT
 *   RIDE THE STREAM (below) driven to the end — submit, advance and wait until nothing runs, read the results in place — on a
 *   pool of its own, one block of as many slots as the largest call so far: no ticket and no slice number of a pending request
 *   moves, and nothing is copied back between the launches.  A call whose pool cannot be allocated fails with MGX_ERR_HIP and
 *   leaves no pool behind: the same requests in smaller calls go through.  results[i] is filled for every
 *   request; the points of request i are path_xy[first_point .. first_point + n_points), requests in order; *n_points = all
 *   points.  point_capacity too small: results (first_point, n_points and the rest) and *n_points are filled, path_xy is not
 *   touched, MGX_ERR_INVALID.  NULL requests / results / n_points, NULL path_xy with a capacity, or a non-finite coordinate:
 *   MGX_ERR_INVALID and nothing is changed.  MGX_ERR_STATE while switched off and on a sharded world (one with ghosts).
 * mgx_plan_tree(w, request, capacity, xy, parent, cost, n_nodes): the tree of a request of the LAST mgx_plan_paths (for tests and
 *   tools): positions [.][2], parents (-1: the root) and stored costs of the first min(capacity, *n_nodes) nodes; any array
 *   may be NULL.
 *
 * PLANS THAT RIDE THE STREAM.  mgx_plan_paths holds its caller until every request has ended — tens of driver ticks.  The
 *   reference starts a path-finding task and polls it once a frame while every other robot keeps ticking (robot.rs:578-799); these
 *   calls are that: requests wait in a pool that outlives a call, a slice of iterations is ENQUEUED on the world's stream, and the
 *   host hears which requests have ended from a completion log the launches append to in host-mapped memory.  A request's arrays
 *   never move while it is pending (the pool grows by blocks of slots), and the plan is mgx_plan_paths' bit for bit: the same
 *   kernel through the same host code, and where the slices fall does not show.  Unsharded worlds, planner on.
 * mgx_plan_submit(w, n, requests, tickets): queues the n requests and returns at once — nothing is launched, nothing waited for.
 *   tickets[i] names request i: counted from 1 per world, never used twice (not after mgx_planner_enable(NULL) either).  Requests
 *   already pending are not disturbed.  MGX_ERR_STATE: planner off, sharded world.  MGX_ERR_INVALID: NULL arguments, a non-finite
 *   coordinate, more than 4096 requests pending — nothing is queued.
 * mgx_plan_advance(w, iterations): enqueues ONE launch that gives every pending request that has not ended at most `iterations`
 *   iterations (growth and smoothing iterations alike), one workgroup each, and does not wait.  Nothing pending: nothing is
 *   launched.  iterations == 0: MGX_ERR_INVALID.  A request's SLICE NUMBER is the count of advances since it was submitted.
 *   HOW MANY SLICES A REQUEST TAKES, with g its `iterations`, s its `smoothing_iterations` and B the budget of every advance:
 *     MGX_PLAN_OK, MGX_PLAN_TREE_FULL: ceil((g + s) / B), and never less than 1 — the launch that makes the last iteration also
 *       writes the points out: the finish takes no budget.
 *     MGX_PLAN_MAX_ITERATIONS: max_iterations / B + 1 in integer division — the limit is seen at the top of an iteration that
 *       still has budget, so a launch that ends exactly on the limit leaves the verdict to the next.
 * mgx_planner_set_tick_budget(w, iterations): 0 (the default) is off.  Otherwise every mgx_mission_tick_end, and so every tick of
 *   mgx_mission_run, ends by enqueuing one such slice behind its own launches when requests are pending — on the SAME stream: a
 *   planner workgroup that ran beside the tick would hold a CU's LDS and make the residency census decline the tick's resident
 *   launch.  A setting of the world: it survives mgx_planner_enable.
 * mgx_plan_collect(w, flags, capacity, done, path_xy, point_capacity, n_done, n_points): hands out requests that have ended, in the
 *   order of (slice number, ticket), each once.  done[i].result is what mgx_plan_paths returns for the request, first_point into
 *   this call's path_xy.  flags 0: what the device has reported so far — it looks at the event behind the last slice
 *   (hipEventQuery) and at the log, and never waits.  MGX_PLAN_WAIT: it first waits for the slices enqueued so far; it advances
 *   nothing itself.  A request that does not fit into what is left of `done` or `path_xy` stays, with those behind it, for the
 *   next call: MGX_OK, *n_done and *n_points say what came.  MGX_ERR_STATE: planner off.
 * mgx_plan_cancel(w, ticket): the request will never be handed out (its robot was despawned while it waited); its slot is used
 *   again once the slices in flight have completed.  MGX_ERR_INVALID: a ticket that is unknown, collected or cancelled.
 * mgx_plan_pending(w, n): requests submitted and neither collected nor cancelled.
 * mgx_planner_enable while requests are pending: env == NULL drops them with everything else; a new map is MGX_ERR_STATE and
 *   changes nothing.  mgx_plan_paths and mgx_plan_tree work beside pending requests (they wait for the slices enqueued, and
 *   advance none of them).
 *
 * A PARAMETER SET PER GROUP.  A launch runs many requests, and the runs of a parameter sweep that share a world (ROBOT GROUPS)
 *   differ in `rrt.*` as they differ in seed or sigmas.  A group here is only the index of a parameter set, 0 ..
 *   MGX_GROUPS_MAX - 1: no robot of that group need exist.  The sets live in one table in device memory, uploaded on the
 *   world's stream when one changes; a request carries the index of its set from submit on, and its workgroup reads the row once
 *   per launch.  A launch none of whose requests names a set is handed no table and runs the code it ran before there were sets.
 * mgx_planner_set_group_params(w, group, params): from the next submit on, requests of `group` run under *params.  params ==
 *   NULL puts the group back on the world's parameters.  Checked in this order, with nothing changed on failure: planner off,
 *   MGX_ERR_STATE; group >= MGX_GROUPS_MAX, MGX_ERR_INVALID; the value checks mgx_planner_enable makes on a parameter struct,
 *   MGX_ERR_INVALID; max_nodes or iterations_per_launch neither 0 nor equal to what the world runs with, MGX_ERR_INVALID — these
 *   two belong to the launch (they fix the LDS size, the arrays' strides and the budget), and a set is stored with the world's;
 *   requests pending (mgx_plan_pending > 0), MGX_ERR_STATE: a set does not change under a request that is running.
 *   sample_half_extent 0 is 2000, as in mgx_planner_enable.  mgx_planner_enable in either form (a new map, or NULL) forgets every
 *   group's set.
 * mgx_planner_group_params(w, group, out): what a request of the group would run under — its own set, or the world's as
 *   mgx_planner_enable took it (defaults filled in).  MGX_ERR_STATE: planner off.  MGX_ERR_INVALID: NULL, group >= MGX_GROUPS_MAX.
 * mgx_plan_paths_groups, mgx_plan_submit_groups: mgx_plan_paths and mgx_plan_submit with one group per request; groups == NULL
 *   is group 0 for every request, and that is what mgx_plan_paths and mgx_plan_submit are.  A group >= MGX_GROUPS_MAX is
 *   MGX_ERR_INVALID and nothing is queued.  On a world that has never set a group's parameters they compute what the plain calls
 *   compute, bit for bit.  Everything else keeps its statement per request: mgx_plan_tree, the collect order (slice number,
 *   ticket), cancel, pending, and HOW MANY SLICES A REQUEST TAKES with the max_iterations of the request's own group.
 *   mgx_plan_done.group is the group a request was submitted under. */
#define MGX_PLAN_OK 0
#define MGX_PLAN_MAX_ITERATIONS 1
#define MGX_PLAN_TREE_FULL 2
typedef struct mgx_plan_params {
    float step_size, neighbourhood_radius, collision_radius; /* RRTSection (config)                          */
    uint32_t max_iterations;
    int32_t smoothing_enabled;
    uint32_t smoothing_max_iterations;
    float smoothing_step;
    float sample_half_extent;       /* 0: 2000, the reference's constant (gbp_global_planner lib.rs:155-185) */
    uint32_t max_nodes;             /* 0: 8192                                                               */
    uint32_t iterations_per_launch; /* 0: 1024                                                               */
} mgx_plan_params;
typedef struct mgx_plan_request {
    float start[2], end[2];
    uint64_t wyrand_state;
} mgx_plan_request;
typedef struct mgx_plan_result {
    int32_t status;                 /* MGX_PLAN_*                                                            */
    uint32_t first_point, n_points; /* into path_xy; 0 points unless status is MGX_PLAN_OK                   */
    uint32_t n_nodes, iterations;
    uint32_t smoothing_iterations;  /* smoothing iterations made (a word that was reserved and 0)            */
    double cost;                    /* of the path before smoothing                                          */
    uint64_t wyrand_state;          /* the stream after the draws made                                       */
} mgx_plan_result;
int mgx_planner_enable(mgx_world *w, const mgx_env_desc *env, const mgx_plan_params *params);
int mgx_plan_paths(mgx_world *w, uint32_t n, const mgx_plan_request *requests, mgx_plan_result *results, float *path_xy,
                   uint32_t point_capacity, uint32_t *n_points);
int mgx_plan_tree(mgx_world *w, uint32_t request, uint32_t capacity, double *xy, int32_t *parent, double *cost,
                  uint32_t *n_nodes);
#define MGX_PLAN_WAIT 1u
typedef struct mgx_plan_done {
    uint64_t ticket;
    uint32_t slices;                /* the slice number it ended in                                          */
    uint32_t group;                 /* the group it was submitted under (a word that was reserved and 0)     */
    mgx_plan_result result;
} mgx_plan_done;
int mgx_plan_submit(mgx_world *w, uint32_t n, const mgx_plan_request *requests, uint64_t *tickets);
int mgx_plan_advance(mgx_world *w, uint32_t iterations);
int mgx_planner_set_tick_budget(mgx_world *w, uint32_t iterations);
int mgx_plan_collect(mgx_world *w, uint32_t flags, uint32_t capacity, mgx_plan_done *done, float *path_xy,
                     uint32_t point_capacity, uint32_t *n_done, uint32_t *n_points);
int mgx_plan_cancel(mgx_world *w, uint64_t ticket);
int mgx_plan_pending(mgx_world *w, uint32_t *n);
int mgx_planner_set_group_params(mgx_world *w, uint32_t group, const mgx_plan_params *params);
int mgx_planner_group_params(mgx_world *w, uint32_t group, mgx_plan_params *out);
int mgx_plan_paths_groups(mgx_world *w, uint32_t n, const mgx_plan_request *requests, const uint32_t *groups,
                          mgx_plan_result *results, float *path_xy, uint32_t point_capacity, uint32_t *n_points);
int mgx_plan_submit_groups(mgx_world *w, uint32_t n, const mgx_plan_request *requests, const uint32_t *groups,
                           uint64_t *tickets);

/* ---- host helpers (no device needed) --------------------------------------------------- */
/* gbp_schedule: fills steps[max(n_int,n_ext)] with MGX_STEP_* bits. Returns the count
 * or a negative status. (crates/gbp_schedule/src/schedules/ *.rs) */
int mgx_schedule(int32_t kind, uint8_t n_internal, uint8_t n_external, uint8_t *steps,
                 uint32_t capacity);
/* get_variable_timesteps (crates/magics/src/utils.rs:35-75). Returns the count. */
int mgx_variable_timesteps(uint32_t lookahead_horizon, uint32_t lookahead_multiple,
                           uint32_t *timesteps, uint32_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H */
