// Test harness: the module shim's geometry on the host, for tests/test_follow_host.py.  Attaches the module to a
// host-only solver handle (gpuDevice = TPC_MPC_DEVICE_NONE: no GPU is looked for), fills the TRAJECTORY channel from a
// file and prints what the shim's own code returns: getTrajectoryPoint, vertex2f::length and
// LookupTable<float>::linearSearch.  Nothing of the walk or the table search is restated here.
//
// usage: follow_harness cases.bin          exit code 3 = initialize() refused
// cases.bin, float32: T, then T tables { m, vx[m], vy[m] }, then N, then N cases
//   { count, look_ahead, car_velocity, count x { x, y, dir_x, dir_y, velocity } }   (count <= 0: an empty trajectory)
// output, one line per case, hex floats: ox oy dir_x dir_y velocity distance, then the model speed under each table.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "trajectory_point_controller.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<float> d;
    float buf[4096];
    for (size_t got; (got = std::fread(buf, sizeof(float), 4096, fh)) > 0;) d.insert(d.end(), buf, buf + got);
    std::fclose(fh);
    size_t at = 0;
    auto next = [&]() -> float { if (at >= d.size()) { std::fprintf(stderr, "short file\n"); std::exit(2); } return d[at++]; };

    lms::ChannelStore channels;
    std::map<std::string, std::shared_ptr<void>> services;
    services["PHOENIX_SERVICE"] = std::make_shared<phoenix_CC2016_service::Phoenix_CC2016Service>();
    TrajectoryPointController mod;
    mod.attach(&channels, &services);
    mod.config().set("gpuDevice", (int)TPC_MPC_DEVICE_NONE);
    if (!mod.initialize()) {
        std::printf("{\"initialize\": false}\n");
        return 3;
    }
    auto traj = channels.get<street_environment::Trajectory>("TRAJECTORY");

    const int T = (int)next();
    std::vector<lms::math::LookupTable<float, lms::math::LookupTableOrder::ASC>> tables(T);
    for (int t = 0; t < T; ++t) {
        const int m = (int)next();
        for (int i = 0; i < m; ++i) tables[t].vx.push_back(next());
        for (int i = 0; i < m; ++i) tables[t].vy.push_back(next());
    }
    const int N = (int)next();
    for (int c = 0; c < N; ++c) {
        const int count = (int)next();
        const float look = next(), carv = next();
        traj->clear();
        for (int i = 0; i < count; ++i) {
            street_environment::TrajectoryPoint p;
            const float x = next(), y = next(), dx = next(), dy = next();
            p.position = lms::math::vertex2f(x, y);
            p.directory = lms::math::vertex2f(dx, dy);
            p.velocity = next();
            traj->push_back(p);
        }
        const street_environment::TrajectoryPoint tp = mod.getTrajectoryPoint(look);
        std::printf("%a %a %a %a %a %a", (double)tp.position.x, (double)tp.position.y, (double)tp.directory.x,
                    (double)tp.directory.y, (double)tp.velocity, (double)tp.position.length());
        double v = carv;                       // cycle()'s clamp in front of the table (the shim's cycleTobiMpc)
        if (std::fabs(v) < 0.1) v = 0.1;
        for (int t = 0; t < T; ++t) std::printf(" %a", (double)tables[t].linearSearch((float)v));
        std::printf("\n");
    }
    mod.deinitialize();
    return 0;
}
