// ray_sets_main.cpp — host/rays.h's offsets and ray_sets as a stand-alone program (tests/test_ray_sets_host.py): one generator
// per run, the result written to stdout as raw rt_ray records.
//   ray_sets_main KIND one  dx dy  ARGS...    the generator with that offset: one record per pixel
//   ray_sets_main KIND sets k 0    ARGS...    rays::ray_sets through Camera::sampleOffsets(k)'s (dx, dy): k records per pixel, ray-major
// KIND and ARGS as rays_main:  equirect w h yaw px py pz | fisheye w h fov yaw pitch px py pz | ortho w h extent yaw pitch px py pz |
// cubemap n px py pz
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../host/rays.h"

static_assert(sizeof(rt_ray) == 32 && alignof(rt_ray) == 16, "rt_ray is two 16-byte groups");

// Camera::sampleOffsets' (dx, dy) restated (host/camera.cpp): the program stands alone, without the host library
static double radical_inverse(unsigned base, unsigned index) {
    double f = 1.0, r = 0.0;
    for (unsigned i = index; i > 0; i /= base) {
        f /= (double)base;
        r += f * (double)(i % base);
    }
    return r;
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const std::string kind = argv[1], mode = argv[2];
    auto num = [&](int i) { return i < argc ? std::atof(argv[i]) : 0.0; };
    const int a0 = 5;   // the first of ARGS
    float pos[3];
    auto pos_at = [&](int i) { for (int k = 0; k < 3; k++) pos[k] = (float)num(i + k); };
    pos_at(kind == "equirect" ? a0 + 3 : kind == "cubemap" ? a0 + 1 : a0 + 5);
    auto generate = [&](rays::Offset off) -> std::vector<rt_ray> {
        if (kind == "equirect") return rays::equirect(pos, (int)num(a0), (int)num(a0 + 1), num(a0 + 2), off);
        if (kind == "fisheye") return rays::fisheye(pos, (int)num(a0), (int)num(a0 + 1), num(a0 + 2), num(a0 + 3), num(a0 + 4), off);
        if (kind == "ortho") return rays::orthographic(pos, (int)num(a0), (int)num(a0 + 1), num(a0 + 2), num(a0 + 3), num(a0 + 4), off);
        if (kind == "cubemap") return rays::cubemap(pos, (int)num(a0), off);
        return {};
    };
    std::vector<rt_ray> r;
    if (mode == "one") {
        r = generate(rays::Offset{num(3), num(4)});
    } else if (mode == "sets") {
        const unsigned k = (unsigned)num(3);
        std::vector<float> offsets;
        for (unsigned j = 0; j < k; j++) {
            offsets.push_back((float)radical_inverse(2, j + 1) - 0.5f);
            offsets.push_back((float)radical_inverse(3, j + 1) - 0.5f);
        }
        r = rays::ray_sets(generate, offsets, 2);
    } else {
        return 2;
    }
    if (r.empty()) return 3;
    return std::fwrite(r.data(), sizeof(rt_ray), r.size(), stdout) == r.size() ? 0 : 1;
}
