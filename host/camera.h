// camera.h — Camera with the reference's public surface (include/camera.h:20-53,
// src/camera.cpp:26-118 of antoni-wojcik/OpenCL-Raytracing), without glm.
// What the trace kernels see of it is transferData(): 12 floats = position,
// lower_left_corner, horizontal, vertical (kernels/raytracer.cl:129-134,503).
#pragma once
#include <cstdint>
#include <vector>

#include "vecmath.h"

enum CameraMovementDirection { FORWARD, BACK, LEFT, RIGHT };

class Camera {
    float fov, aspect;
    float speed;
    float half_height, half_width;
    float yaw, pitch;
    rth::vec3 u, v, w;
    rth::vec3 position;
    rth::vec3 horizontal, vertical, lower_left_corner;

    void updateVectors();
    void setFov();

public:
    Camera(int camera_fov, float camera_aspect, const rth::vec3 &pos = rth::vec3(0.0f, 0.0f, 0.0f), float y = 0.0f,
           float p = 0.0f);

    void move(CameraMovementDirection dir, float dt);
    void rotate(float x, float y);
    void zoom(float scroll);

    void setFasterSpeed(bool speed_up);
    void setSlowerSpeed(bool speed_down);
    void setSize(float new_aspect);

    // pointer to a function-static float[12]: valid until the next call, not thread-safe
    // (the reference's contract, src/camera.cpp:94-110)
    float *transferData() const;

    // n x 12 floats: one camera block per sample first_sample .. first_sample + n - 1, for RayTracer::renderSamplesCameras
    // (rt_render_spp_cameras) — pixel jitter (anti-aliasing) and / or a thin lens (depth of field).  Block j, in float and
    // in this order, with i = first_sample + j + 1 the index into the Halton sequences:
    //     hor' = F * horizontal, ver' = F * vertical                       (F = focus; only with aperture != 0)
    //     off = a * (lx * u + ly * v)                                       (a = aperture; (lx, ly) the lens point)
    //     position' = position + off
    //     llc' = (F * llc + (dx / width) * hor' + (dy / height) * ver') - off
    // (dx, dy) = Halton(2, 3)(i) - 0.5; (lx, ly) = sqrt(h5) * (cos, sin)(2 pi h7), (h5, h7) = Halton(5, 7)(i); the radical
    // inverses in double, rounded once.  A term that is switched off is not computed: with jitter off and aperture 0
    // every block is transferData().  The same arithmetic as camera.py's sampleBlocks, bit for bit.
    std::vector<float> sampleBlocks(uint32_t n, uint32_t first_sample, int width, int height, bool pixel_jitter = true,
                                    float aperture = 0.0f, float focus = 1.0f) const;
    // n x 4 floats: (dx, dy, lx, ly) of sampleBlocks for samples first_sample .. first_sample + n - 1 (camera.py's
    // sampleOffsets): the pixel offsets and lens points of rays::ray_sets
    static std::vector<float> sampleOffsets(uint32_t n, uint32_t first_sample = 0);
    // van der Corput radical inverse of `index` in `base`
    static double radicalInverse(uint32_t base, uint32_t index);
};
