"""Trackers on the device: a robot that joins BETWEEN mgx_mission_tick_begin and _end — the missions are laid out again inside the
tick's second half, the tracker state is keyed by robot id and is not: the others' timers, previous samples and distances go on,
the newcomer starts from zero and is sampled in the tick it joined."""
import numpy as np
import pytest

from magics_amd import World, scenarios as S

from test_gpu_tracks import PERIOD, Checker, _device_samples

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("reserve", [True, False], ids=["appended", "relayout"])
def test_a_robot_joins_between_the_two_halves_of_a_tick(reserve):
    n, K, ticks, join = 6, 10, 12, 5
    sc = S.circle_scenario(n, K, circle_radius=12.0, n_internal=10, n_external=10)
    sc["ir"] = []
    w = World(sc["params"])
    if reserve:
        w.reserve(n + 2)
    assert S.populate(w, dict(sc, robots=sc["robots"][:n - 1])) == list(range(n - 1))
    dt32 = F(1.0) / F(10.0)
    ts = np.array([float(dt32 / F(rb["t0"])) for rb in sc["robots"]])

    def mission(r):
        rb = sc["robots"][r]
        r2, cur = float(F(rb["radius"]) * F(rb["radius"])), rb["mean0"][0]
        w.mission_set(r, np.asarray([tuple(rb["goal"])], dtype=np.float64), K - 1, 0, r2, r2, (F(cur[0]), F(0.5), F(cur[1])), ts[r])
    for r in range(n - 1):
        mission(r)
    w.tracks_enable(True, period_ns=PERIOD, tick_ns=PERIOD, next_tick=0)
    own, chk, nn = np.zeros(n), Checker(n, PERIOD), 1
    for k in range(ticks):
        m0, m1 = w.read_variable_means(0), w.read_variable_means(1)
        old = np.arange(len(m0))
        nn, _, _, fin = w.mission_tick_begin(12.0, nn)
        assert not len(fin)
        if k == join:
            rb = sc["robots"][n - 1]
            assert w.add_robot(rb["mean0"], rb["prior_diag"], rb["dt"], rb["radius"], path=rb["path"], order_key=rb["order_key"]) == n - 1
            mission(n - 1)
        w.mission_tick_end(sc["steps"], float(F(sc["target_speed"])), float(dt32))
        change = ts[old, None] * (m1[old] - m0[old])
        own[old] += np.sqrt(change[:, 0] * change[:, 0] + change[:, 1] * change[:, 1])      # (driver.py, Driver.tick)
        tr = np.zeros((n, 3), F)
        got = w.mission_read()[0]
        tr[:len(got)] = got
        if k == join:  # the newcomer moved in the tick it joined: its first increment, as far as its Transform shows it
            start = np.array([sc["robots"][n - 1]["mean0"][0][0], sc["robots"][n - 1]["mean0"][0][1]])
            moved = float(np.hypot(float(tr[n - 1, 0]) - start[0], float(tr[n - 1, 2]) - start[1]))
            samples, in_log, dropped, dist = w.tracks_take(capacity=0)               # (too little room: nothing is taken)
            assert len(samples) == 0 and in_log == (n - 1) * (join + 1) + 1 and dropped == 0
            assert moved > 0 and abs(dist[n - 1] - moved) <= 1e-4 * moved
            own[n - 1] = dist[n - 1]
        chk.step(k, range(n - 1 if k < join else n), tr)
    got, in_log, dropped, dist = w.tracks_take()
    assert dropped == 0 and _device_samples(got) == chk.samples
    assert np.array_equal(dist, own) and (dist > 0).all()
    new = [s for s in chk.samples if s[1] == n - 1]
    assert new[0][0] == join and new[0][4] == 0 and all(s[4] == 1 for s in new[1:])
    assert all(s[4] == 1 for s in chk.samples if s[1] < n - 1 and s[0] > 0)              # nobody else started again
    appends = w.append_stats()
    assert appends[0] >= 1 if reserve else appends[:2] == (0, 0), appends
