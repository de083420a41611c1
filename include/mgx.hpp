// mgx.hpp — C++ host side above the C ABI (include/mgx.h), shaped like the reference's Rust API so
// that code written against `magics`' FactorGraph reads the same here: the reference is compiled
// code (Rust, no toolchain in this image), so the native mirror is C++; `rust/magics-hip` carries
// the same thing as Rust source, `magics_amd/world.py` as Python.  Header-only, no dependencies
// beyond the C ABI.  Invariant violations that panic in the reference throw mgx::Error here;
// lookups that return Option return std::optional.
//
// Reference interfaces mirrored (paths under crates/magics/src unless noted):
//   FactorGraph            factorgraph/factorgraph.rs:74-76,190-226,304-353,380-436,494-528,688-826,876-890
//   VariableNode (belief)  factorgraph/variable.rs:40-54,140-166
//   iterate_gbp_v2         planner/robot.rs:1769-1861          GbpSchedule  crates/gbp_schedule
//   topology systems       planner/robot.rs:1362-1601          RobotNumberGenerator planner/robot.rs:122-140
//   MultivariateNormal     crates/gbp_multivariate_normal/src/lib.rs:38-410
#pragma once

#include <array>
#include <cstdint>
#include <limits>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mgx.h"

namespace mgx {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};
inline int check(int rc) {
    if (rc < 0) throw Error(rc, mgx_last_error());
    return rc;
}

using Vector4 = std::array<double, 4>;
using Matrix4 = std::array<double, 16>;  // row-major

// VariableNode.belief (variable.rs:40-54)
struct Belief {
    Vector4 information_vector, mean;
    Matrix4 precision_matrix, covariance_matrix;
    bool valid;
    std::array<double, 2> estimated_position() const { return {mean[0], mean[1]}; }
    std::array<double, 2> estimated_velocity() const { return {mean[2], mean[3]}; }
};

// MessagesSent / MessagesReceived (factorgraph/mod.rs:29-137)
struct MessageCount {
    uint64_t sent_internal, sent_external, received_internal, received_external;
};

// crates/gbp_schedule: one step of the interleaved schedule
struct GbpScheduleAtIteration {
    bool internal, external;
};
enum class GbpSchedule : int32_t {
    Centered = MGX_SCHEDULE_CENTERED,
    SoonAsPossible = MGX_SCHEDULE_SOON_AS_POSSIBLE,
    LateAsPossible = MGX_SCHEDULE_LATE_AS_POSSIBLE,
    InterleaveEvenly = MGX_SCHEDULE_INTERLEAVE_EVENLY,
    HalfBeginningHalfEnd = MGX_SCHEDULE_HALF_BEGINNING_HALF_END,
};
inline std::vector<GbpScheduleAtIteration> schedule(GbpSchedule kind, uint8_t internal, uint8_t external) {
    uint8_t steps[256];
    const int n = check(mgx_schedule(static_cast<int32_t>(kind), internal, external, steps, 256));
    std::vector<GbpScheduleAtIteration> out((size_t)n);
    for (int i = 0; i < n; i++) out[(size_t)i] = {(steps[i] & MGX_STEP_INTERNAL) != 0, (steps[i] & MGX_STEP_EXTERNAL) != 0};
    return out;
}
// utils.rs:35-75
inline std::vector<uint32_t> get_variable_timesteps(uint32_t lookahead_horizon, uint32_t lookahead_multiple) {
    uint32_t ts[1024];
    const int n = check(mgx_variable_timesteps(lookahead_horizon, lookahead_multiple, ts, 1024));
    return std::vector<uint32_t>(ts, ts + n);
}

/// the map's colliders in the reference's creation order (mgx_env_colliders): tile cuboids, then the placeable obstacles
struct EnvColliders {
    std::vector<mgx_env_collider> colliders;
    std::vector<std::array<float, 2>> vertices;  ///< the polygons' world (x, z) vertices, counter-clockwise
};
inline EnvColliders env_colliders(const mgx_env_desc &env) {
    EnvColliders out;
    uint32_t n = 0, nv = 0;
    check(mgx_env_colliders(&env, nullptr, 0, &n, nullptr, 0, &nv));
    out.colliders.resize(n);
    out.vertices.resize(nv);
    if (n) check(mgx_env_colliders(&env, out.colliders.data(), n, &n, nv ? out.vertices[0].data() : nullptr, nv, &nv));
    return out;
}

class World;

// The reference's `FactorGraph` component: here a handle (world, robot id).  Message routing happens
// on the device, so the calls that return message vectors in the reference return nothing.
class FactorGraph {
public:
    int32_t id() const { return robot_; }
    void internal_factor_iteration();
    void internal_variable_iteration();
    void change_prior_of_variable(uint32_t variable_index, const Vector4 &mean);
    void delete_interrobot_factors_connected_to(const FactorGraph &other);
    std::optional<Belief> get_variable(uint32_t variable_index) const;
    std::optional<Belief> nth_variable(uint32_t i) const { return get_variable(i); }
    std::optional<Belief> first_variable() const { return get_variable(0); }
    std::optional<Belief> last_variable() const;
    MessageCount message_count() const;
    void set_antenna_active(bool active);
    void set_idle(bool idle);
    /// modify_tracking_factors(|t| t.set_tracking_path(path)) (factorgraph.rs:1467, tracking.rs:134-136; robot.rs:674-682):
    /// two points or more; the tracking factors keep their records and timeouts
    void set_tracking_path(const std::vector<std::array<float, 2>> &path);

private:
    friend class World;
    FactorGraph(World *w, int32_t robot) : world_(w), robot_(robot) {}
    World *world_;
    int32_t robot_;
};

// planner/robot.rs:122-140
struct RobotNumberGenerator {
    uint64_t next_value = 1;
    uint64_t next() { return next_value++; }
    void reset() { next_value = 1; }
};

class World {
public:
    explicit World(const mgx_params &params) { check(mgx_world_create(&params, &w_)); }
    ~World() { if (w_) mgx_world_destroy(w_); }
    World(const World &) = delete;
    World &operator=(const World &) = delete;
    mgx_world *raw() const { return w_; }

    void set_sdf(const std::vector<uint8_t> &rgb, uint32_t width, uint32_t height, double world_w, double world_h) {
        if (rgb.size() != (size_t)width * height * 3) throw Error(MGX_ERR_INVALID, "rgb size does not match width x height x 3");
        check(mgx_world_set_sdf(w_, rgb.data(), width, height, world_w, world_h));
    }
    // RobotBundle::new (robot.rs:1134-1356): K variables, their initial means, prior diagonal, delta_t
    FactorGraph add_robot(const std::vector<Vector4> &mean0, const std::vector<double> &prior_diag, const std::vector<double> &delta_t,
                          double radius, uint64_t order_key, const std::vector<std::array<float, 2>> &path = {}, uint32_t group = 0) {
        if (prior_diag.size() != mean0.size() || delta_t.size() + 1 != mean0.size()) throw Error(MGX_ERR_INVALID, "inconsistent sizes");
        mgx_robot_desc d{};
        d.group = group;  // the independent run the robot belongs to (mgx.h, ROBOT GROUPS)
        d.K = (uint32_t)mean0.size();
        d.n_path = (uint32_t)path.size();
        d.mean0 = mean0[0].data();
        d.prior_diag = prior_diag.data();
        d.dt = delta_t.data();
        d.path_xy = path.empty() ? nullptr : path[0].data();
        d.radius = radius;
        d.order_key = order_key;
        int32_t id = -1;
        check(mgx_robot_add(w_, &d, &id));
        K_ = d.K;
        return FactorGraph(this, id);
    }
    void remove_robot(const FactorGraph &g) { check(mgx_robot_remove(w_, g.id())); }

    // create_interrobot_factors, one direction (robot.rs:1500-1585)
    void connect(const FactorGraph &owner, const FactorGraph &other, RobotNumberGenerator &numbers) {
        check(mgx_ir_connect(w_, owner.id(), other.id(), numbers.next_value));
        numbers.next_value += K_ - 1;
    }
    // update_robot_neighbours + delete_ + create_interrobot_factors (robot.rs:1362-1586);
    // translations: Transform::translation of every robot (x, y, z as f32), id order
    /// One FixedUpdate tick of the planner chain (robot.rs:86-103): both prior updates for the listed robots, then
    /// iterate_gbp_v2 over `steps` — one call, the prior updates ride in the launch that opens the tick
    void tick(const std::vector<int32_t> &robots, const std::vector<double> &waypoints_xy, const std::vector<double> &time_scale,
              const std::vector<uint8_t> &what, double max_speed, double delta_t, const std::vector<uint8_t> &steps) {
        check(mgx_tick(w_, (uint32_t)robots.size(), robots.data(), waypoints_xy.data(), time_scale.data(), what.data(), max_speed,
                       delta_t, steps.data(), (uint32_t)steps.size()));
    }
    /// how the last iterate_gbp_v2 / tick ran: sweep-kernel launches (1 = the whole schedule as one resident launch)
    uint32_t last_launch_count() {
        uint32_t n = 0;
        check(mgx_last_launch_count(w_, &n));
        return n;
    }
    /// everything issued so far is enqueued: a lingering launch is told to end (no wait); how long launches linger (us, 0: never)
    void flush() { check(mgx_flush(w_)); }
    void set_linger(int32_t microseconds) { check(mgx_set_linger(w_, microseconds)); }
    /// 0: every resident launch in the full form of the kernel; 1: the smallest form that covers it (default); which one ran last
    void set_specialize(int32_t enabled) { check(mgx_set_specialize(w_, enabled)); }
    uint32_t last_sweep_features() { uint32_t f = 0; check(mgx_last_sweep_features(w_, &f)); return f; }
    /// back-to-back schedules merged into one post: 0 off, 1 while the launch is behind (default), 2 whenever they fit
    void set_post_merge(int32_t mode) { check(mgx_set_post_merge(w_, mode)); }
    /// FactorGraph::change_factor_enabled (factorgraph.rs:1529-1539) for every graph: MGX_FACTOR_* bits
    void change_factor_enabled(uint32_t kind_mask) { check(mgx_set_enabled(w_, kind_mask)); }
    /// FactorGraph::update_inter_robot_safety_distance_multiplier (factorgraph.rs:892-910) for every graph and for factors
    /// created from now on, as ui/settings.rs:586-590 applies it: finite and > 0
    void update_inter_robot_safety_distance_multiplier(double multiplier) { check(mgx_set_safety_multiplier(w_, multiplier)); }
    std::pair<uint32_t, uint32_t> update_topology(const std::vector<std::array<float, 3>> &translations, float comms_radius,
                                                  RobotNumberGenerator &numbers) {
        uint32_t stats[2] = {0, 0};
        check(mgx_update_topology(w_, translations[0].data(), comms_radius, MGX_NEIGHBOURS_AUTO, &numbers.next_value, stats));
        return {stats[0], stats[1]};
    }
    // the same pass on a grouped world (mgx.h, ROBOT GROUPS): one generator per group; {created, deleted} per group
    std::vector<std::pair<uint32_t, uint32_t>> update_topology_groups(const std::vector<std::array<float, 3>> &translations, float comms_radius,
                                                                      std::vector<RobotNumberGenerator> &numbers) {
        std::vector<uint64_t> next(numbers.size());
        for (size_t g = 0; g < numbers.size(); g++) next[g] = numbers[g].next_value;
        std::vector<uint32_t> stats(2 * numbers.size() + 2, 0u);
        check(mgx_update_topology_groups(w_, translations[0].data(), comms_radius, MGX_NEIGHBOURS_AUTO, (uint32_t)numbers.size(), next.data(), stats.data()));
        std::vector<std::pair<uint32_t, uint32_t>> out(numbers.size());
        for (size_t g = 0; g < numbers.size(); g++) {
            numbers[g].next_value = next[g];
            out[g] = {stats[2 * g], stats[2 * g + 1]};
        }
        return out;
    }
    // ... with one comms radius per group (comms_radii.size() == numbers.size())
    std::vector<std::pair<uint32_t, uint32_t>> update_topology_groups(const std::vector<std::array<float, 3>> &translations,
                                                                      const std::vector<float> &comms_radii, std::vector<RobotNumberGenerator> &numbers) {
        if (comms_radii.size() != numbers.size()) throw std::invalid_argument("one comms radius per group");
        std::vector<uint64_t> next(numbers.size());
        for (size_t g = 0; g < numbers.size(); g++) next[g] = numbers[g].next_value;
        std::vector<uint32_t> stats(2 * numbers.size() + 2, 0u);
        check(mgx_update_topology_groups_radii(w_, translations[0].data(), comms_radii.data(), MGX_NEIGHBOURS_AUTO, (uint32_t)numbers.size(), next.data(),
                                               stats.data()));
        std::vector<std::pair<uint32_t, uint32_t>> out(numbers.size());
        for (size_t g = 0; g < numbers.size(); g++) {
            numbers[g].next_value = next[g];
            out[g] = {stats[2 * g], stats[2 * g + 1]};
        }
        return out;
    }
    // iterate_gbp_v2 (robot.rs:1769-1861)
    void iterate_gbp_v2(const std::vector<GbpScheduleAtIteration> &sched) {
        std::vector<uint8_t> steps(sched.size());
        for (size_t i = 0; i < sched.size(); i++) steps[i] = (uint8_t)((sched[i].internal ? MGX_STEP_INTERNAL : 0) | (sched[i].external ? MGX_STEP_EXTERNAL : 0));
        check(mgx_iterate(w_, steps.data(), (uint32_t)steps.size()));
    }
    /// iterate_gbp_v2 with one schedule per robot group (mgx_iterate_groups): group g runs per_group[g], an empty one sits the call out
    void iterate_gbp_v2_groups(const std::vector<std::vector<GbpScheduleAtIteration>> &per_group) {
        std::vector<uint8_t> steps;
        std::vector<uint32_t> first(1, 0u);
        for (const auto &sched : per_group) {
            for (const GbpScheduleAtIteration &s : sched) steps.push_back((uint8_t)((s.internal ? MGX_STEP_INTERNAL : 0) | (s.external ? MGX_STEP_EXTERNAL : 0)));
            first.push_back((uint32_t)steps.size());
        }
        check(mgx_iterate_groups(w_, (uint32_t)per_group.size(), steps.data(), first.data()));
    }
    /// calls that ran MIXED (groups with different schedules), the sweep-kernel launches of those calls, workgroups that sat one out
    std::array<uint64_t, 3> group_schedule_stats() {
        std::array<uint64_t, 3> s{};
        check(mgx_group_schedule_stats(w_, &s[0], &s[1], &s[2]));
        return s;
    }
    /// gbp.factors-enabled of ONE robot group (mgx_set_group_enabled): before the group's first robot is added; the inter-robot bit is the world's
    void set_group_enabled(uint32_t group, uint32_t kind_mask) { check(mgx_set_group_enabled(w_, group, kind_mask)); }
    uint32_t group_enabled(uint32_t group) {
        uint32_t m = 0;
        check(mgx_get_group_enabled(w_, group, &m));
        return m;
    }
    /// schedules that ran as group plans only because the world is masked, and the sweep-kernel launches of those
    std::array<uint64_t, 2> group_enabled_stats() {
        std::array<uint64_t, 2> s{};
        check(mgx_group_enabled_stats(w_, &s[0], &s[1]));
        return s;
    }
    /// a masked world's equal schedules as resident launches of the masked form (mgx_set_group_resident; off by default)
    void set_group_resident(bool enabled) { check(mgx_set_group_resident(w_, enabled ? 1 : 0)); }
    /// resident launches of the masked form, schedules posted into one, schedules that ran as group plans all the same
    std::array<uint64_t, 3> group_resident_stats() {
        std::array<uint64_t, 3> s{};
        check(mgx_group_resident_stats(w_, &s[0], &s[1], &s[2]));
        return s;
    }
    /// gbp.sigma-factor-* of ONE robot group (mgx_set_group_sigmas): before the group's first robot is added; equal to the world's is none
    void set_group_sigmas(uint32_t group, const mgx_group_sigmas &s) { check(mgx_set_group_sigmas(w_, group, &s)); }
    mgx_group_sigmas group_sigmas(uint32_t group) {
        mgx_group_sigmas s{};
        check(mgx_get_group_sigmas(w_, group, &s));
        return s;
    }
    /// several iterate_gbp_v2 calls, one submission (mgx_batch_begin / mgx_batch_end): `{ auto b = world.batch(); for (...) world.iterate_gbp_v2(s); }`
    struct Batch {
        mgx_world *w;
        uint32_t schedules = 0, launches = 0;
        explicit Batch(mgx_world *world) : w(world) { check(mgx_batch_begin(w)); }
        Batch(const Batch &) = delete;
        Batch &operator=(const Batch &) = delete;
        void end() { if (w) { mgx_world *x = w; w = nullptr; check(mgx_batch_end(x, &schedules, &launches)); } }
        ~Batch() { if (w) (void)mgx_batch_end(w, nullptr, nullptr); }
    };
    Batch batch() { return Batch(w_); }
    // update_prior_of_horizon_state + update_prior_of_current_state_v3 (robot.rs:2182-2338)
    void update_priors(const std::vector<int32_t> &robots, const std::vector<std::array<double, 2>> &next_waypoints,
                       const std::vector<double> &time_scale, double max_speed, double delta_t) {
        std::vector<uint8_t> what(robots.size(), 3);
        check(mgx_update_priors(w_, (uint32_t)robots.size(), robots.data(), next_waypoints[0].data(), time_scale.data(), what.data(),
                                max_speed, delta_t));
    }
    /// The path-finding completion handler (robot.rs:643-799) for a batch of robots in one call (mgx_apply_global_paths):
    /// set_tracking_path, reset_variables(means, first_last_sigma, inbetween_sigma), and per `flags` (MGX_GLOBAL_PATH_*)
    /// reset_tracking_factors, the device mission's new route paths[i][1:] and mission.state = Active.  means[i]: K vectors.
    /// In place on the device for a laid-out, unsharded world that never switched a factor kind; the per-robot calls otherwise.
    void apply_global_paths(const std::vector<int32_t> &robots, const std::vector<std::vector<std::array<float, 2>>> &paths,
                            const std::vector<std::vector<Vector4>> &means, double first_last_sigma = 1e30,
                            double inbetween_sigma = std::numeric_limits<double>::infinity(),
                            uint32_t flags = MGX_GLOBAL_PATH_RESET_TRACKING) {
        if (paths.size() != robots.size() || means.size() != robots.size()) throw Error(MGX_ERR_INVALID, "one path and one set of means per robot");
        std::vector<uint32_t> ptr(robots.size() + 1, 0);
        std::vector<float> xy;
        std::vector<double> m;
        for (size_t i = 0; i < robots.size(); i++) {
            for (const auto &p : paths[i]) { xy.push_back(p[0]); xy.push_back(p[1]); }
            ptr[i + 1] = (uint32_t)(xy.size() / 2);
            if (means[i].size() != (size_t)K_) throw Error(MGX_ERR_INVALID, "means: one vector per variable");
            for (const Vector4 &v : means[i]) m.insert(m.end(), v.begin(), v.end());
        }
        check(mgx_apply_global_paths(w_, (uint32_t)robots.size(), robots.data(), ptr.data(), xy.data(), m.data(), first_last_sigma,
                                     inbetween_sigma, flags));
    }
    /// (full rebuilds of the device arrays from the host mirror, downloads of the device state into it) — mgx_layout_stats
    std::pair<uint64_t, uint64_t> layout_stats() {
        uint64_t layouts = 0, pulls = 0;
        check(mgx_layout_stats(w_, &layouts, &pulls));
        return {layouts, pulls};
    }
    /// head-room for robots that join while the world runs: they are appended on the device instead of laid out again — mgx_world_reserve
    void reserve(uint32_t robots) { check(mgx_world_reserve(w_, robots)); }
    /// (commits that appended in place, robots they brought onto the device, commits that fell back to the full layout) — mgx_append_stats
    std::array<uint64_t, 3> append_stats() {
        uint64_t appends = 0, robots = 0, fallbacks = 0;
        check(mgx_append_stats(w_, &appends, &robots, &fallbacks));
        return {appends, robots, fallbacks};
    }
    std::vector<Vector4> read_variable_means(uint32_t variable_index) {
        uint32_t n = 0;
        check(mgx_num_robots(w_, &n, nullptr));
        std::vector<Vector4> out(n);
        if (n) check(mgx_read_variable_means(w_, variable_index, out[0].data()));
        return out;
    }
    /// update_robot_robot_collisions on the device (planner/collisions.rs:72-140): while enabled every mission tick ends with one
    /// pass; `update` is the same pass over Transforms the caller keeps; `read` is the one call that waits for the device
    void collisions_enable(bool enabled = true, uint32_t method = MGX_NEIGHBOURS_AUTO, uint64_t event_capacity = 0) {
        check(mgx_collisions_enable(w_, enabled ? 1 : 0, method, event_capacity));
    }
    void collisions_update(const std::vector<std::array<float, 3>> &translations) { check(mgx_collisions_update(w_, translations[0].data())); }
    struct Collisions {
        std::vector<mgx_collision_event> events;  ///< from `first` on, in (pass, robot_a, robot_b) order
        uint64_t n_total = 0, dropped = 0;
        std::vector<uint32_t> per_robot;
    };
    Collisions collisions_read(uint64_t first = 0) {
        Collisions out;
        uint32_t n = 0;
        check(mgx_num_robots(w_, &n, nullptr));
        out.per_robot.assign(n, 0u);
        check(mgx_collisions_read(w_, first, nullptr, 0, &out.n_total, &out.dropped, nullptr));
        out.events.resize(out.n_total > first ? (size_t)(out.n_total - first) : 0);
        check(mgx_collisions_read(w_, first, out.events.data(), out.events.size(), &out.n_total, &out.dropped, out.per_robot.data()));
        return out;
    }
    void collisions_clear() { check(mgx_collisions_clear(w_)); }
    /// update_robot_environment_collisions on the device (planner/collisions.rs:368-438) against the colliders of `env`
    /// (env_colliders above); nullptr switches it off.  `update` / `read` / `clear` as for the robot-robot pass.
    void env_collisions_enable(const mgx_env_desc *env, uint64_t event_capacity = 0) { check(mgx_env_collisions_enable(w_, env, event_capacity)); }
    void env_collisions_update(const std::vector<std::array<float, 3>> &translations) {
        check(mgx_env_collisions_update(w_, translations.empty() ? nullptr : translations[0].data()));  // (empty: the device's Transforms)
    }
    struct EnvCollisions {
        std::vector<mgx_env_collision_event> events;  ///< from `first` on, in (pass, robot, collider) order
        uint64_t n_total = 0, dropped = 0;
        std::vector<uint32_t> per_robot;
    };
    EnvCollisions env_collisions_read(uint64_t first = 0) {
        EnvCollisions out;
        uint32_t n = 0;
        check(mgx_num_robots(w_, &n, nullptr));
        out.per_robot.assign(n, 0u);
        check(mgx_env_collisions_read(w_, first, nullptr, 0, &out.n_total, &out.dropped, nullptr));
        out.events.resize(out.n_total > first ? (size_t)(out.n_total - first) : 0);
        check(mgx_env_collisions_read(w_, first, out.events.data(), out.events.size(), &out.n_total, &out.dropped, out.per_robot.data()));
        return out;
    }
    void env_collisions_clear() { check(mgx_env_collisions_clear(w_)); }
    /// goal areas on the device (goal_area.rs:67-103, specified in mgx.h): while enabled every mission tick ends with one pass that
    /// records the first arrival of every robot in every area; `update` is the same pass over Transforms the caller keeps at a
    /// tick the caller names; `read` is the one call that waits for the device.  No areas: off
    void goal_areas_enable(const std::vector<mgx_goal_area> &areas, uint64_t next_tick = 0) {
        check(mgx_goal_areas_enable(w_, areas.empty() ? nullptr : areas.data(), (uint32_t)areas.size(), next_tick));
        goal_areas_ = (uint32_t)areas.size();
    }
    void goal_areas_set_clock(uint64_t next_tick) { check(mgx_goal_areas_set_clock(w_, next_tick)); }
    void goal_areas_update(uint64_t tick, const std::vector<std::array<float, 3>> &translations) {
        check(mgx_goal_areas_update(w_, translations.empty() ? nullptr : translations[0].data(), tick));  // (empty: the device's Transforms)
    }
    struct GoalArrivals {
        std::vector<mgx_goal_arrival> arrivals;  ///< every arrival, in (tick, robot, area) order
        std::vector<uint32_t> per_area;
    };
    GoalArrivals goal_areas_read() {
        GoalArrivals out;
        uint64_t total = 0;
        out.per_area.assign(goal_areas_, 0u);
        check(mgx_goal_areas_read(w_, nullptr, 0, &total, out.per_area.data()));
        out.arrivals.resize((size_t)total);
        if (total) check(mgx_goal_areas_read(w_, out.arrivals.data(), out.arrivals.size(), &total, out.per_area.data()));
        return out;
    }
    void goal_areas_clear() { check(mgx_goal_areas_clear(w_)); }
    /// the trackers on the device (planner/tracking.rs:117-136, 210-240, specified in mgx.h): while enabled every mission tick ends
    /// with one pass — a sample of every moving robot every `period_ns` and its distance travelled; `update` is the sampling pass
    /// over Transforms the caller keeps; `take` is the one call that waits for the device and empties the log
    void tracks_enable(bool enabled, uint64_t period_ns, uint64_t tick_ns, uint64_t next_tick = 0, uint64_t sample_capacity = 0) {
        check(mgx_tracks_enable(w_, enabled ? 1 : 0, period_ns, tick_ns, next_tick, sample_capacity));
    }
    void tracks_set_clock(uint64_t next_tick) { check(mgx_tracks_set_clock(w_, next_tick)); }
    void tracks_update(uint64_t tick, const std::vector<std::array<float, 3>> &translations, const std::vector<uint8_t> &moved) {
        check(mgx_tracks_update(w_, translations.empty() ? nullptr : translations[0].data(), moved.empty() ? nullptr : moved.data(), tick));
    }
    struct Tracks {
        std::vector<mgx_track_sample> samples;  ///< the whole log, in (tick, robot) order
        uint64_t dropped = 0;
        std::vector<double> travelled;          ///< per robot
    };
    Tracks tracks_take() {
        Tracks out;
        uint32_t n = 0;
        uint64_t taken = 0, in_log = 0;
        check(mgx_num_robots(w_, &n, nullptr));
        out.travelled.assign(n, 0.0);
        check(mgx_tracks_take(w_, nullptr, 0, &taken, &in_log, &out.dropped, nullptr));
        out.samples.resize((size_t)in_log);
        check(mgx_tracks_take(w_, out.samples.data(), out.samples.size(), &taken, &in_log, &out.dropped, out.travelled.data()));
        out.samples.resize((size_t)taken);
        return out;
    }
    void tracks_clear() { check(mgx_tracks_clear(w_)); }
    void tracks_set_logging(bool on) { check(mgx_tracks_set_logging(w_, on ? 1 : 0)); }
    /// run metrics (mgx_track_metrics_*, specified in mgx.h): dimensionless jerk and path deviation per robot, carried by the
    /// tracker pass; `read` is the one call that waits, LDJ = -log(dimensionless_jerk)
    void track_metrics_enable(bool enabled, uint32_t max_route_points = 0) { check(mgx_track_metrics_enable(w_, enabled ? 1 : 0, max_route_points)); }
    void track_metrics_set_route(int32_t robot, const std::vector<std::array<double, 2>> &xy) {
        check(mgx_track_metrics_set_route(w_, robot, xy.empty() ? nullptr : xy[0].data(), (uint32_t)xy.size()));
    }
    std::vector<mgx_track_metrics> track_metrics_read() {
        uint32_t n = 0;
        check(mgx_num_robots(w_, &n, nullptr));
        std::vector<mgx_track_metrics> out(n);
        check(mgx_track_metrics_read(w_, out.data(), out.size()));
        return out;
    }
    /// the global planner (batched RRT* over the colliders of `env`, specified in mgx.h); nullptr switches it off
    void planner_enable(const mgx_env_desc *env, const mgx_plan_params &params) { check(mgx_planner_enable(w_, env, &params)); }
    struct Plans {
        std::vector<mgx_plan_result> results;     ///< one per request; its points are path_xy[first_point .. + n_points)
        std::vector<std::array<float, 2>> path_xy;
    };
    /// groups: one group per request (empty: group 0 for all) — the parameter set each runs under (planner_set_group_params)
    Plans plan_paths(const std::vector<mgx_plan_request> &requests, const std::vector<uint32_t> &groups = {}) {
        if (!groups.empty() && groups.size() != requests.size()) throw std::invalid_argument("plan_paths: one group per request");
        const uint32_t *g = groups.empty() ? nullptr : groups.data();
        Plans out;
        out.results.resize(requests.size());
        out.path_xy.resize(256 * requests.size() + 1);
        uint32_t total = 0;
        int rc = mgx_plan_paths_groups(w_, (uint32_t)requests.size(), requests.data(), g, out.results.data(), out.path_xy[0].data(), (uint32_t)out.path_xy.size(), &total);
        if (rc == MGX_ERR_INVALID && total > out.path_xy.size()) {  // (the counts came back: once more with room for them)
            out.path_xy.resize(total);
            rc = mgx_plan_paths_groups(w_, (uint32_t)requests.size(), requests.data(), g, out.results.data(), out.path_xy[0].data(), total, &total);
        }
        check(rc);
        out.path_xy.resize(total);
        return out;
    }
    /// plans that ride the stream (mgx.h): submit returns tickets at once, advance enqueues one slice for every pending request,
    /// collect hands out what has ended — in the order of (slice number, ticket), each once; wait = false never blocks
    std::vector<uint64_t> plan_submit(const std::vector<mgx_plan_request> &requests, const std::vector<uint32_t> &groups = {}) {
        if (!groups.empty() && groups.size() != requests.size()) throw std::invalid_argument("plan_submit: one group per request");
        std::vector<uint64_t> tickets(requests.size());
        check(mgx_plan_submit_groups(w_, (uint32_t)requests.size(), requests.data(), groups.empty() ? nullptr : groups.data(), tickets.data()));
        return tickets;
    }
    /// a parameter set per group (mgx.h): requests of `group` run under `params` from the next submit on; nullptr: the world's again
    void planner_set_group_params(uint32_t group, const mgx_plan_params *params) { check(mgx_planner_set_group_params(w_, group, params)); }
    mgx_plan_params planner_group_params(uint32_t group) {
        mgx_plan_params out{};
        check(mgx_planner_group_params(w_, group, &out));
        return out;
    }
    void plan_advance(uint32_t iterations) { check(mgx_plan_advance(w_, iterations)); }
    void planner_set_tick_budget(uint32_t iterations) { check(mgx_planner_set_tick_budget(w_, iterations)); }
    struct PlansDone {
        std::vector<mgx_plan_done> done;          ///< result.first_point .. + n_points index path_xy
        std::vector<std::array<float, 2>> path_xy;
    };
    PlansDone plan_collect(bool wait = false, uint32_t capacity = 64, uint32_t point_capacity = 4096) {
        PlansDone out;
        out.done.resize(capacity);
        out.path_xy.resize((size_t)point_capacity + 1);
        uint32_t n_done = 0, n_points = 0;
        check(mgx_plan_collect(w_, wait ? MGX_PLAN_WAIT : 0u, capacity, out.done.data(), out.path_xy[0].data(), point_capacity, &n_done, &n_points));
        out.done.resize(n_done);
        out.path_xy.resize(n_points);
        return out;
    }
    void plan_cancel(uint64_t ticket) { check(mgx_plan_cancel(w_, ticket)); }
    uint32_t plan_pending() {
        uint32_t n = 0;
        check(mgx_plan_pending(w_, &n));
        return n;
    }
    void synchronize() { check(mgx_synchronize(w_)); }
    uint32_t K() const { return K_; }

private:
    mgx_world *w_ = nullptr;
    uint32_t K_ = 0;
    uint32_t goal_areas_ = 0;  // areas handed to goal_areas_enable (the size of per_area)
};

inline void FactorGraph::internal_factor_iteration() { check(mgx_internal_factor_iteration(world_->raw(), robot_)); }
inline void FactorGraph::internal_variable_iteration() { check(mgx_internal_variable_iteration(world_->raw(), robot_)); }
inline void FactorGraph::change_prior_of_variable(uint32_t ix, const Vector4 &mean) { check(mgx_change_prior(world_->raw(), robot_, ix, mean.data())); }
inline void FactorGraph::delete_interrobot_factors_connected_to(const FactorGraph &other) { check(mgx_ir_disconnect(world_->raw(), robot_, other.robot_)); }
inline std::optional<Belief> FactorGraph::get_variable(uint32_t ix) const {
    if (ix >= world_->K()) return std::nullopt;
    Belief b{};
    int32_t valid = 0;
    check(mgx_get_belief(world_->raw(), robot_, ix, b.information_vector.data(), b.precision_matrix.data(), b.mean.data(),
                         b.covariance_matrix.data(), &valid));
    b.valid = valid != 0;
    return b;
}
inline std::optional<Belief> FactorGraph::last_variable() const { return world_->K() ? get_variable(world_->K() - 1) : std::nullopt; }
inline MessageCount FactorGraph::message_count() const {
    uint64_t c[4];
    check(mgx_message_counts(world_->raw(), robot_, c));
    return {c[0], c[1], c[2], c[3]};
}
inline void FactorGraph::set_antenna_active(bool active) { check(mgx_set_antenna(world_->raw(), robot_, active ? 1 : 0)); }
inline void FactorGraph::set_idle(bool idle) { check(mgx_set_idle(world_->raw(), robot_, idle ? 1 : 0)); }
inline void FactorGraph::set_tracking_path(const std::vector<std::array<float, 2>> &path) {
    check(mgx_set_tracking_path(world_->raw(), robot_, path.empty() ? nullptr : path[0].data(), (uint32_t)path.size()));
}

// crates/gbp_multivariate_normal: errors are the variants of MultivariateNormalError, carried by
// mgx::Error::code (MGX_MVN_ERR_*) and what()
class MultivariateNormal {
public:
    static MultivariateNormal from_information_and_precision(const std::vector<double> &information, const std::vector<double> &precision,
                                                             uint32_t rows, uint32_t cols) {
        mgx_mvn *m = nullptr;
        check(mgx_mvn_from_information_and_precision(information.data(), (uint32_t)information.size(), precision.data(), rows, cols, &m));
        return MultivariateNormal(m);
    }
    static MultivariateNormal from_mean_and_covariance(const std::vector<double> &mean, const std::vector<double> &covariance,
                                                       uint32_t rows, uint32_t cols) {
        mgx_mvn *m = nullptr;
        check(mgx_mvn_from_mean_and_covariance(mean.data(), (uint32_t)mean.size(), covariance.data(), rows, cols, &m));
        return MultivariateNormal(m);
    }
    size_t len() const { return mgx_mvn_len(m_.get()); }
    std::vector<double> information_vector() const { std::vector<double> v(len()); check(mgx_mvn_get(m_.get(), v.data(), nullptr, nullptr)); return v; }
    std::vector<double> precision_matrix() const { std::vector<double> v(len() * len()); check(mgx_mvn_get(m_.get(), nullptr, v.data(), nullptr)); return v; }
    std::vector<double> mean() const { std::vector<double> v(len()); check(mgx_mvn_get(m_.get(), nullptr, nullptr, v.data())); return v; }
    std::vector<double> covariance() const { std::vector<double> v(len() * len()); check(mgx_mvn_covariance(m_.get(), v.data())); return v; }
    bool update() { return check(mgx_mvn_update(m_.get())) == 1; }
    void set_information_vector(const std::vector<double> &v) { check(mgx_mvn_set_information_vector(m_.get(), v.data())); }
    void set_precision_matrix(const std::vector<double> &v) { check(mgx_mvn_set_precision_matrix(m_.get(), v.data())); }
    MultivariateNormal operator+(const MultivariateNormal &o) const { return combine(o, MGX_MVN_ADD); }
    MultivariateNormal operator-(const MultivariateNormal &o) const { return combine(o, MGX_MVN_SUB); }
    MultivariateNormal operator*(const MultivariateNormal &o) const { return combine(o, MGX_MVN_MUL); }
    MultivariateNormal &operator+=(const MultivariateNormal &o) { check(mgx_mvn_combine_assign(m_.get(), o.m_.get(), MGX_MVN_ADD)); return *this; }
    MultivariateNormal &operator-=(const MultivariateNormal &o) { check(mgx_mvn_combine_assign(m_.get(), o.m_.get(), MGX_MVN_SUB)); return *this; }
    MultivariateNormal &operator*=(const MultivariateNormal &o) { check(mgx_mvn_combine_assign(m_.get(), o.m_.get(), MGX_MVN_MUL)); return *this; }

private:
    struct Del { void operator()(mgx_mvn *p) const { mgx_mvn_destroy(p); } };
    explicit MultivariateNormal(mgx_mvn *m) : m_(m) {}
    MultivariateNormal combine(const MultivariateNormal &o, int op) const {
        mgx_mvn *m = nullptr;
        check(mgx_mvn_combine(m_.get(), o.m_.get(), op, &m));
        return MultivariateNormal(m);
    }
    std::unique_ptr<mgx_mvn, Del> m_;
};

}  // namespace mgx
