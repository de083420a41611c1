// mgx_world.hip — host side of the C ABI (include/mgx.h): world arena, topology -> slot tables,
// device buffers, launch sequencing.  No CPU compute path exists: every compute entry point
// needs a HIP device.
//
// Host keeps a per-robot / per-connection mirror of all mutable state only to (re)build the
// device arrays when the topology changes (`commit`): device is the source of truth between
// commits; `pull` downloads it first so that added robots / inter-robot connections never
// disturb existing state (the reference mutates its graphs in place,
// factorgraph.rs:190-226,304-353,380-436).
//
// ONE translation unit, sixteen files: the parts below share file-local helpers (commit, confirm_resident, flush_counts, sweep,
// run_resident, linger_close ...) that have no business in the library's symbol table, so they are included here in
// dependency order instead of being linked:
//   mgx_world_types.h — what the host side is made of: launcher prototypes of the kernel files, error text, device buffers, the pinned argument ring, the neighbour search's and the resident launches' state, the host mirror's records (Robot, IrConn), connection sets and index, the world itself, the entry hooks of the C ABI (MGX_ENTER)
//   mgx_resident.h — resident launches, the host's arithmetic, free of HIP (included by mgx_world_types.h): a schedule's segments, their bytes in a launch's plan, parity and segment count, the back-off, riding prior updates
//   mgx_world_mirror.inc — SoA helpers, blob <-> host mirror, pull (device -> host mirror)
//   mgx_world_counters.inc — message counters (MessageCount): the launch log, lazy settling of the connections, flush_counts
//   mgx_world_commit.inc — commit (host mirror -> device arrays), the connection index, the incoming tables, retopo (edge tables rebuilt on the device)
//   mgx_world_launch.inc — launches: confirm_resident, sweep, resident schedule launches, lingering launches (the host's side)
//   mgx_world_abi.inc — C ABI: lifecycle, environment, robots, connections, factor kinds, flags
//   mgx_world_topology.inc — C ABI: dynamic inter-robot topology — neighbour search, delete / create_interrobot_factors
//   mgx_world_observers.inc — what the observers (the three parts below) share: the robots' radii, staged positions and flags, "sharded", the growth of arrays that follow the robots, the checks of an _update call, the observers' end of a tick
//   mgx_world_collisions.inc — C ABI: robot-robot and robot-environment collision bookkeeping on the device, one contact book under both (the passes mgx_mission_tick_end enqueues)
//   mgx_world_tracks.inc — C ABI: the trackers on the device — position / velocity samples and distance travelled (the pass mgx_mission_tick_end enqueues beside the collision passes)
//   mgx_world_goal_areas.inc — C ABI: goal areas on the device — the first arrival of every robot in every area (the pass mgx_mission_tick_end enqueues beside the collision passes)
//   mgx_world_planner.inc — C ABI: the global planner — the map it plans over, batched RRT* requests in bounded launches, the trees read back
//   mgx_world_missions.inc — C ABI: missions on the device, many ticks per call, fine-grained sweeps, schedules -> launches
//   mgx_world_schedule.inc — C ABI: batches, mgx_iterate, prior changes, mgx_tick, resets, diagnostics, read-back
//   mgx_world_shard.inc — C ABI: sharded worlds — exchange lists, migration, the in-engine transports (RCCL, direct, ghost records inside resident launches), hipIpc, pack / unpack
#include "mgx_world_types.h"
#include "mgx_world_mirror.inc"
#include "mgx_world_counters.inc"
#include "mgx_world_commit.inc"
#include "mgx_world_launch.inc"
#include "mgx_world_abi.inc"
#include "mgx_world_topology.inc"
#include "mgx_world_observers.inc"
#include "mgx_world_collisions.inc"
#include "mgx_world_tracks.inc"
#include "mgx_world_goal_areas.inc"
#include "mgx_world_planner.inc"
#include "mgx_world_missions.inc"
#include "mgx_world_schedule.inc"
#include "mgx_world_shard.inc"
