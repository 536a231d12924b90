/*
 * iaf_noise_client.c -- a plain C program (no Python, no torch) that draws noise through include/iaf_hip.h: create a source,
 * fill 8 floats, print them.  TEST CODE: built and run by tests/test_hip_noise.py (gpu-marked), which compares the printed
 * numbers with the known-answer vector of the header (seed 0, substream 0, step 0, elements 0..7).
 *
 *   usage: iaf_noise_client          prints "z <8 floats>" and "step <counter after the fill>"; exit 0 = every call returned IAF_OK
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>

#include "iaf_hip.h"

#define CHECK_HIP(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "HIP error %d at line %d\n", (int)_e, __LINE__); return 2; } } while (0)
#define CHECK_IAF(e) do { int _r = (e); if (_r != IAF_OK) { fprintf(stderr, "iaf error %d (%s) at line %d\n", _r, iaf_error_string(_r), __LINE__); return 3; } } while (0)

int main(void) {
    if (iaf_device_count() < 1) { fprintf(stderr, "no device\n"); return 1; }
    iaf_rng_t* rng = NULL;
    float* d = NULL;
    float h[8];
    CHECK_IAF(iaf_rng_create(&rng, 0));
    CHECK_HIP(hipMalloc((void**)&d, sizeof(h)));
    float* outs[1];
    const size_t counts[1] = {8};
    const unsigned substreams[1] = {0};
    uint64_t step = 99;
    outs[0] = d;
    if (iaf_rng_fill_normal(rng, outs, counts, substreams, NULL, 0, 1, NULL) != IAF_ERR_SHAPE) { fprintf(stderr, "n = 0 accepted\n"); return 4; }
    CHECK_IAF(iaf_rng_fill_normal(rng, outs, counts, substreams, NULL, 1, 1, NULL));
    CHECK_IAF(iaf_rng_tell(rng, &step, NULL));
    CHECK_HIP(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
    printf("z");
    for (int i = 0; i < 8; ++i) printf(" %.7f", h[i]);
    printf("\nstep %llu\n", (unsigned long long)step);
    CHECK_HIP(hipFree(d));
    CHECK_IAF(iaf_rng_destroy(rng));
    return 0;
}
