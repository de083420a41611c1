// Test-only host build of the run metrics' lane arithmetic (magics_amd/csrc/mgx_track_metrics.h, the functions k_tracks_pass and
// k_track_metrics_read call) behind a C interface: tests/test_track_metrics.py drives it sample by sample beside the Python
// streaming form and compares f64 bit patterns.  Built twice, with -ffp-contract=off and -ffp-contract=fast: the header keeps
// its own setting.
#include <cstring>

#include "../../magics_amd/csrc/mgx_track_metrics.h"

using namespace mgx;

extern "C" {

unsigned tm_state_size() { return (unsigned)sizeof(TrackMetricsState); }
unsigned tm_record_size() { return (unsigned)sizeof(TrackMetricsOut); }

void tm_velocity(void *state, double u, double w) {
    TrackMetricsState s;
    memcpy(&s, state, sizeof s);
    track_metrics_velocity(s, u, w);
    memcpy(state, &s, sizeof s);
}

void tm_position(void *state, double px, double py, const double *route_xy, unsigned n_points) {
    TrackMetricsState s;
    memcpy(&s, state, sizeof s);
    track_metrics_position(s, px, py, route_xy, n_points);
    memcpy(state, &s, sizeof s);
}

void tm_read(const void *state, void *record) {  // the state is const: finalisation works on a copy
    TrackMetricsState s;
    memcpy(&s, state, sizeof s);
    const TrackMetricsOut o = track_metrics_finalise(s);
    memcpy(record, &o, sizeof o);
}

}  // extern "C"
