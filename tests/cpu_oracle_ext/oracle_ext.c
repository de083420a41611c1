/* The CPU oracle plus the two run-time mutators it lacks: ONE translation unit — the oracle's source, untouched, and two
 * functions that edit the state it defines.  Built by tests/oracle_ext.py with the flags of oracle/Makefile's default target;
 * a library made from it has every orc_* symbol of the stock oracle, and as long as neither new function is called it
 * computes bit for bit what the stock oracle computes (tests/test_oracle_ext.py). */
#include "../../oracle/gbp_oracle.c"

/* FactorGraph::update_inter_robot_safety_distance_multiplier (FG/factorgraph.rs:892-910) ->
 * InterRobotFactor::update_safety_distance (FG/factor/interrobot.rs:87-89: safety_distance = multiplier * robot_radius),
 * applied as its only caller applies it (ui/settings.rs:586-590): the config entry first — factors created later read it
 * (ROBOT:1506, interrobot.rs:64) — then every graph.  StrictlyPositiveFinite: finite and > 0. */
int orc_set_safety_multiplier(World *w, double multiplier) {
    if (!w || !isfinite(multiplier) || !(multiplier > 0.0)) return ORC_ERR_INVALID;
    w->p.safety_multiplier = multiplier;
    for (int r = 0; r < w->n; r++) {
        Graph *g = &w->g[r];
        for (int i = 0; i < g->n_nodes; i++) {
            Node *nd = &g->nodes[i];
            if (nd->alive && nd->is_factor && nd->f.kind == K_INTERROBOT) nd->f.safety_distance = multiplier * g->radius;
        }
    }
    return ORC_OK;
}

/* FactorGraph::modify_tracking_factors(|t| t.set_tracking_path(path)) (FG/factorgraph.rs:1467, FG/factor/tracking.rs:134-136;
 * the completion handler's first call, ROBOT:674-682).  The graph's tracking factors all follow the graph's polyline here, so
 * the call replaces that; record, last_measurement and timeout of every factor stay (tracking.rs:134-136 assigns the path and
 * nothing else).  TwoOrMore: n_path >= 2. */
int orc_set_tracking_path(World *w, int32_t r, const float *path_xy, uint32_t n_path) {
    if (!w || r < 0 || r >= w->n || !path_xy || n_path < 2 || w->g[r].removed || w->g[r].ghost) return ORC_ERR_INVALID;
    Graph *g = &w->g[r];
    float *p = (float *)malloc(sizeof(float) * 2 * (size_t)n_path);
    memcpy(p, path_xy, sizeof(float) * 2 * (size_t)n_path);
    free(g->path);
    g->path = p;
    g->n_path = (int)n_path;
    return ORC_OK;
}
