// Host-only driver for asan_host.sh: every C-ABI call here returns before any kernel launch (queries, tuning, argument checks).
#include <stdio.h>
#include <string.h>
#include "sempyr.h"

static int fails = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAIL %s (%s)\n", what, sp_last_error_string()); ++fails; } } while (0)

int main(void) {
    EXPECT(sp_version() == SP_VERSION, "version");
    // tuning table: every key settable, out-of-range keys rejected
    for (int k = 0; k < SP_TUNE_COUNT; ++k) { EXPECT(sp_set_tuning(k, 1) == SP_OK, "set_tuning"); EXPECT(sp_set_tuning(k, -1) == SP_OK, "reset"); }
    EXPECT(sp_set_tuning(-1, 0) == SP_ERR_INVALID && sp_set_tuning(SP_TUNE_COUNT, 0) == SP_ERR_INVALID, "set_tuning range");
    EXPECT(strlen(sp_last_error_string()) > 0, "error string");
    // workspace planners over the layer shapes of the step (batch 2 / 20 / 32, channel factors 0.5 / 1 / 2 / 4) and odd ones
    const int batches[] = {1, 2, 3, 20, 32};
    const int chans[] = {3, 8, 16, 64, 65, 72, 128, 136, 256, 264, 512, 520, 768, 1024, 1536};
    const int maps[] = {2, 4, 8, 16, 32, 64, 128, 256};
    long queries = 0;
    for (int dt = 0; dt < 2; ++dt)
        for (unsigned b = 0; b < sizeof(batches) / sizeof(int); ++b)
            for (unsigned i = 0; i < sizeof(chans) / sizeof(int); ++i)
                for (unsigned o = 0; o < sizeof(chans) / sizeof(int); ++o)
                    for (unsigned m = 0; m < sizeof(maps) / sizeof(int); ++m)
                        for (int k = 1; k <= 3; k += 2) {
                            const int e = dt == SP_F32 ? 4 : 8;
                            const int cin_p = (chans[i] + e - 1) / e * e;
                            if ((long)batches[b] * maps[m] * maps[m] * cin_p > (1L << 28)) continue;
                            int64_t bytes = -1, floats = -1;
                            for (int det = 0; det < 2; ++det) {
                                sp_set_tuning(SP_TUNE_DETERMINISTIC, det);
                                EXPECT(sp_conv2d_workspace(batches[b], maps[m], maps[m], cin_p, chans[o], k, dt, &bytes) == SP_OK && bytes >= 0, "conv workspace");
                                EXPECT(sp_conv2d_wgrad_workspace(batches[b], maps[m], maps[m], cin_p, chans[o], k, dt, &floats) == SP_OK && floats >= 0, "wgrad workspace");
                                queries += 2;
                            }
                            // the route query on the same shape, with and without the scratch the query above sized (pointers are never read)
                            sp_conv_params q;
                            memset(&q, 0, sizeof q);
                            q.x = q.w = q.y = &queries;
                            q.n = batches[b]; q.h = q.w_ = maps[m]; q.cin_p = cin_p; q.cout = q.ldy = chans[o]; q.ksize = k; q.dtype = dt;
                            for (int lend = 0; lend < 2; ++lend) {
                                const char* route = NULL;
                                q.workspace = lend ? &queries : NULL; q.workspace_bytes = lend ? bytes : 0; q.split_sync = lend ? (int32_t*)&queries : NULL;
                                EXPECT(sp_conv2d_route(&q, &route) == SP_OK && route != NULL && strlen(route) > 0, "conv route");
                                ++queries;
                            }
                            // the weight gradient's route on the same shape: one group, pooled, two groups; with and without the scratch
                            for (int form = 0; form < 3 && batches[b] > (form == 2); ++form)
                                for (int lend = 0; lend < 2; ++lend) {
                                    const char* route = NULL;
                                    const int rc = sp_conv2d_wgrad_route(batches[b], form == 2 ? (batches[b] + 1) / 2 : 0, maps[m], maps[m], cin_p, chans[o], (chans[o] + e - 1) / e * e,
                                                                         k, form == 1, lend, lend ? floats : 0, dt, &route);
                                    if (form == 0) EXPECT(rc == SP_OK && route != NULL && strlen(route) > 0, "wgrad route");
                                    else EXPECT(rc == SP_ERR_INVALID ? strlen(sp_last_error_string()) > 0 : (rc == SP_OK && route != NULL && strlen(route) > 0), "wgrad route (pooled / pair)");
                                    ++queries;
                                }
                            sp_set_tuning(SP_TUNE_DETERMINISTIC, -1);
                        }
    // argument-check failure paths of the launching entry points (they return before touching the device)
    sp_conv_params p;
    memset(&p, 0, sizeof p);
    EXPECT(sp_conv2d_igemm(NULL, NULL) == SP_ERR_INVALID, "null params");
    EXPECT(sp_conv2d_igemm(&p, NULL) == SP_ERR_INVALID, "null tensors");
    int dummy;
    p.x = p.w = &dummy; p.y = &dummy;
    p.ksize = 5; EXPECT(sp_conv2d_igemm(&p, NULL) == SP_ERR_INVALID, "ksize");
    p.ksize = 3; p.n = 1; p.h = 8; p.w_ = 32; p.cin_p = 12; p.cout = 64; p.ldy = 64; p.dtype = SP_BF16;
    EXPECT(sp_conv2d_igemm(&p, NULL) == SP_ERR_INVALID, "cin_p multiple");
    p.cin_p = 16; p.ldy = 32; EXPECT(sp_conv2d_igemm(&p, NULL) == SP_ERR_INVALID, "ldy");
    p.ldy = 64; p.dtype = 7; EXPECT(sp_conv2d_igemm(&p, NULL) == SP_ERR_INVALID, "dtype");
    p.dtype = SP_BF16; p.pool2 = 3; EXPECT(sp_conv2d_igemm(&p, NULL) == SP_ERR_INVALID, "pool2 range");
    p.pool2 = 1; p.cout = 24; p.ldy = 24; EXPECT(sp_conv2d_igemm(&p, NULL) == SP_ERR_INVALID, "pool2 shape");
    p.pool2 = 0; p.in_up2 = 1; p.ksize = 1; EXPECT(sp_conv2d_igemm(&p, NULL) == SP_ERR_INVALID, "in_up2 shape");
    const char* route = NULL;
    p.in_up2 = 0; p.ksize = 3; p.cout = 64; p.ldy = 64; p.tail_w = p.tail_y = &dummy; p.tail_cout = 3; p.tail_ld = 3;
    EXPECT(sp_conv2d_route(&p, &route) == SP_ERR_UNSUPPORTED, "route: tail on 8 rows");
    EXPECT(sp_conv2d_route(NULL, &route) == SP_ERR_INVALID && sp_conv2d_route(&p, NULL) == SP_ERR_INVALID, "route null");
    int64_t out;
    EXPECT(sp_conv2d_workspace(0, 8, 8, 8, 8, 3, SP_BF16, &out) == SP_ERR_INVALID, "workspace bad dims");
    EXPECT(sp_conv2d_wgrad_workspace(1, 8, 8, 8, 8, 2, SP_BF16, &out) == SP_ERR_INVALID, "wgrad workspace bad ksize");
    EXPECT(sp_conv2d_wgrad_route(2, 0, 8, 32, 16, 16, 16, 3, 0, 0, 0, SP_BF16, NULL) == SP_ERR_INVALID, "wgrad route null");
    EXPECT(sp_conv2d_wgrad_route(2, 2, 8, 32, 16, 16, 16, 3, 0, 0, 0, SP_BF16, &route) == SP_ERR_INVALID, "wgrad route split == n");
    EXPECT(sp_conv2d_wgrad_route(2, 1, 8, 32, 12, 16, 16, 3, 0, 0, 0, SP_BF16, &route) == SP_ERR_INVALID, "wgrad route pair cin_p multiple");
    EXPECT(sp_conv2d_wgrad_route(2, 0, 8, 32, 16, 16, 16, 5, 0, 0, 0, SP_BF16, &route) == SP_ERR_INVALID, "wgrad route ksize");
    EXPECT(sp_conv2d_wgrad_route(2, 0, 8, 32, 16, 16, 16, 3, 0, 0, 0, 7, &route) == SP_ERR_INVALID, "wgrad route dtype");
    EXPECT(sp_conv2d_wgrad_route(2, 0, 8, 32, 16, 24, 16, 3, 0, 0, 0, SP_BF16, &route) == SP_ERR_INVALID, "wgrad route cout > ld_dy");
    EXPECT(sp_conv2d_wgrad_route(2, 0, 8, 32, 16, 16, 16, 3, 1, 0, 0, SP_F32, &route) == SP_ERR_INVALID, "wgrad route pooled fp32");
    EXPECT(sp_conv2d_wgrad_route(2, 0, 8, 24, 16, 16, 16, 3, 1, 0, 0, SP_BF16, &route) == SP_ERR_INVALID, "wgrad route pooled w % 32");
    EXPECT(sp_conv2d_wgrad_accum(NULL, NULL, NULL, NULL, NULL, 0, 2, 8, 32, 16, 16, 16, 3, SP_BF16, NULL) == SP_ERR_INVALID, "wgrad_accum null");
    EXPECT(sp_conv2d_wgrad_accum_pair(&dummy, &dummy, (float*)&dummy, NULL, (float*)&dummy, NULL, NULL, 0, 2, 1, 8, 32, 12, 16, 16, 3, 0, SP_BF16, NULL) == SP_ERR_INVALID,
           "wgrad_accum_pair cin_p multiple");
    EXPECT(sp_conv2d_wgrad_accum_pooled(&dummy, &dummy, (float*)&dummy, NULL, NULL, 0, 2, 8, 24, 16, 16, 16, 3, SP_BF16, NULL) == SP_ERR_INVALID, "wgrad_accum_pooled w % 32");
    const char* bwd = NULL;
    EXPECT(sp_attention_route(70, 256, 64, 160, SP_BF16, &route, &bwd) == SP_OK && strcmp(route, "mfma") == 0 && strcmp(bwd, "mfma") == 0, "attention route mfma");
    EXPECT(sp_attention_route(70, 256, 64, 240, SP_BF16, &route, &bwd) == SP_OK && strcmp(route, "mfma") == 0 && strcmp(bwd, "valu tq16") == 0, "attention route mixed");
    EXPECT(sp_attention_route(70, 256, 64, 176, SP_F32, &route, &bwd) == SP_OK && strcmp(route, "valu tq32") == 0 && strcmp(bwd, "valu tq32") == 0, "attention route fp32");
    EXPECT(sp_attention_route(70, 257, 64, 64, SP_BF16, &route, &bwd) == SP_ERR_INVALID, "attention route nk");
    EXPECT(sp_attention_route(70, 256, 64, 64, SP_BF16, NULL, &bwd) == SP_ERR_INVALID, "attention route null");
    printf("asan_driver: %ld planner queries, %d failures\n", queries, fails);
    return fails != 0;
}
