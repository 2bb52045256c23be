// ray_queries_main K SEED OFFSET < n x 6 floats (point, normal) > n x K rt_ray records: rays::hemisphere_sets of host/rays.h
// as a stand-alone program, for tests/test_ray_queries_host.py (compared with opencl-raytracing_amd/rays.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../host/rays.h"

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const unsigned long k = std::strtoul(argv[1], nullptr, 10);
    const unsigned long long seed = std::strtoull(argv[2], nullptr, 0);
    const double offset = std::strtod(argv[3], nullptr);
    std::vector<float> points, normals;
    float rec[6];
    while (std::fread(rec, sizeof(float), 6, stdin) == 6) {
        points.insert(points.end(), rec, rec + 3);
        normals.insert(normals.end(), rec + 3, rec + 6);
    }
    const std::vector<rt_ray> sets = rays::hemisphere_sets(points, normals, (uint32_t)k, seed, offset);
    if (sets.empty() || sets.size() != points.size() / 3 * k) return 3;   // (bad arguments give an empty batch)
    return std::fwrite(sets.data(), sizeof(rt_ray), sets.size(), stdout) == sets.size() ? 0 : 1;
}
