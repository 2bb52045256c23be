// rays_main.cpp — host/rays.h as a stand-alone program (tests/test_rays_host.py): one generator per run, the batch written
// to stdout as raw rt_ray records.
//   rays_main equirect  w h yaw            px py pz
//   rays_main fisheye   w h fov yaw pitch  px py pz
//   rays_main ortho     w h extent yaw pitch px py pz
//   rays_main cubemap   n                  px py pz
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../host/rays.h"

static_assert(sizeof(rt_ray) == 32 && alignof(rt_ray) == 16, "rt_ray is two 16-byte groups");

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string kind = argv[1];
    auto num = [&](int i) { return i < argc ? std::atof(argv[i]) : 0.0; };
    auto pos_at = [&](int i, float p[3]) { for (int k = 0; k < 3; k++) p[k] = (float)num(i + k); };
    float pos[3];
    std::vector<rt_ray> r;
    if (kind == "equirect") { pos_at(5, pos); r = rays::equirect(pos, (int)num(2), (int)num(3), num(4)); }
    else if (kind == "fisheye") { pos_at(7, pos); r = rays::fisheye(pos, (int)num(2), (int)num(3), num(4), num(5), num(6)); }
    else if (kind == "ortho") { pos_at(7, pos); r = rays::orthographic(pos, (int)num(2), (int)num(3), num(4), num(5), num(6)); }
    else if (kind == "cubemap") { pos_at(3, pos); r = rays::cubemap(pos, (int)num(2)); }
    else return 2;
    if (r.empty()) return 3;
    return std::fwrite(r.data(), sizeof(rt_ray), r.size(), stdout) == r.size() ? 0 : 1;
}
