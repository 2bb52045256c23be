// scene_prep_main.cpp — csrc/scene_prep.hpp as a stand-alone host program (tests/test_scene_prep_cpp.py builds it with
// g++ under AddressSanitizer and UBSan): reads a flat scene file, prepares the scene as rt_set_scene does, runs the
// self-check and prints its eight numbers (stats[0..6] in decimal, the digest in hex).
// File: ten uint32 (the counts of rt_scene_desc in its order, then 0), then the nine arrays in rt_scene_desc's order.
#include <cstdio>
#include <string>
#include <vector>

#include "scene_prep.hpp"

template <class T>
static bool read_array(FILE *f, std::vector<T> &v, uint32_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s scene.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t c[10];
    std::vector<rt_material> materials;
    std::vector<rt_sphere> spheres;
    std::vector<rt_plane> planes;
    std::vector<rt_lens> lenses;
    std::vector<rt_float3> vertices;
    std::vector<rt_float2> uvs;
    std::vector<uint32_t> indices;
    std::vector<rt_mesh> meshes;
    std::vector<rt_model> models;
    bool ok = fread(c, 4, 10, f) == 10 && read_array(f, materials, c[0]) && read_array(f, spheres, c[1]) &&
              read_array(f, planes, c[2]) && read_array(f, lenses, c[3]) && read_array(f, vertices, c[4]) &&
              read_array(f, uvs, c[5]) && read_array(f, indices, c[6]) && read_array(f, meshes, c[7]) &&
              read_array(f, models, c[8]) && fgetc(f) == EOF;
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: not a flat scene file\n", argv[1]); return 2; }
    // (an empty vector's data() may be NULL, as an empty array of the C ABI may be)
    rt_scene_desc d = {materials.data(), spheres.data(), planes.data(), lenses.data(), vertices.data(), uvs.data(),
                       indices.data(), meshes.data(), models.data(), c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], 0};
    scene_prep::PreparedScene ps;
    std::string err;
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc = scene_prep::prepare_scene(d, ps, err);
    if (rc == RT_OK) rc = scene_prep::check_prepared(d, ps, stats, err);
    if (rc != RT_OK) { fprintf(stderr, "error %d: %s\n", rc, err.c_str()); return 1; }
    for (int i = 0; i < 7; i++) printf("%llu ", (unsigned long long)stats[i]);
    printf("0x%016llx\n", (unsigned long long)stats[7]);
    return 0;
}
