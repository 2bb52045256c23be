/* A C program that includes rt_amd.h and names the two ray queries: it must compile as C and link against librt_amd.so
 * (tests/test_ray_queries_host.py).  Run without a device it only checks the argument rules that need none. */
#include <stdio.h>

#include "../../include/rt_amd.h"

int main(void) {
    int (*hit)(rt_context *, const void *, size_t, const rt_feature_chain_params *, void *) = rt_intersect_rays;
    int (*occ)(rt_context *, const void *, size_t, uint32_t, const float *, float, void *) = rt_occluded_rays;
    const int a = hit(NULL, NULL, 1, NULL, NULL), b = occ(NULL, NULL, 1, 1, NULL, 1.0f, NULL);
    printf("%d %d\n", a, b);
    return a == RT_EINVAL && b == RT_EINVAL ? 0 : 1;
}
