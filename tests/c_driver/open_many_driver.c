/* Plain-C consumer of zigz_merkle_open_many (include/zigz_hip.h): commit two tables in one batch, open three leaves in one
 * call, hand the four output arrays plus heights straight to zigz_merkle_verify_batch, and compare one opening with
 * zigz_merkle_open_batch.  No Python, no torch, no oracle.
 * Exit code 0 = every check passed (prints "open_many_driver: ok"), 77 = no GPU, 1 = a check failed.
 */
#include <stdio.h>
#include <string.h>
#include <stdint.h>

#include "zigz_hip.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                                   \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            failures++;                                                                                    \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                    \
            printf(__VA_ARGS__);                                                                           \
            printf("\n");                                                                                  \
        }                                                                                                  \
    } while (0)

int main(void) {
    static const uint64_t t0[5] = {1, 2, 3, 4, 5}, t1[1] = {7}; /* heights 3 (padded to 8) and 0 */
    const uint64_t *tables[2] = {t0, t1};
    const size_t ns[2] = {5, 1};
    const uint32_t trees[3] = {0, 1, 0};
    const uint64_t indices[3] = {1, 0, 4};
    const uint64_t one_each[2] = {1, 0};
    uint8_t batch_roots[64], sib[6 * 32], dirs[6], roots[3 * 32], verdicts[3], sib1[3 * 32], dirs1[3];
    uint64_t leaves[3], leaves1[2];
    size_t heights[3], batch_heights[2], rejected = 99, bad = 99;
    zigz_merkle_batch *b = NULL;
    zigz_ctx *ctx = NULL;
    int ndev = 0;
    zigz_status st;

    if (zigz_device_count(&ndev) != ZIGZ_OK || ndev == 0) {
        printf("open_many_driver: no GPU\n");
        return 77;
    }
    st = zigz_ctx_create(0, &ctx);
    CHECK(st == ZIGZ_OK && ctx, "ctx_create: %d", (int)st);
    if (!ctx) return 1;
    st = zigz_merkle_commit_batch(ctx, tables, ns, 2, batch_roots, batch_heights, &b, NULL);
    CHECK(st == ZIGZ_OK && b && batch_heights[0] == 3 && batch_heights[1] == 0, "commit_batch: %d", (int)st);
    if (b) {
        memset(sib, 0xEE, sizeof sib);
        st = zigz_merkle_open_many(ctx, b, 3, trees, indices, sib, dirs, leaves, roots, heights, &bad);
        CHECK(st == ZIGZ_OK, "open_many: %d (%s)", (int)st, zigz_last_error(ctx));
        CHECK(heights[0] == 3 && heights[1] == 0 && heights[2] == 3, "heights");
        CHECK(leaves[0] == 2 && leaves[1] == 7 && leaves[2] == 5, "leaves");
        CHECK(dirs[0] == 1 && dirs[1] == 0 && dirs[2] == 0 && dirs[3] == 0 && dirs[4] == 0 && dirs[5] == 1, "dirs");
        CHECK(!memcmp(roots, batch_roots, 32) && !memcmp(roots + 32, batch_roots + 32, 32) && !memcmp(roots + 64, batch_roots, 32), "roots");
        st = zigz_merkle_verify_batch(ctx, 3, roots, heights, leaves, sib, dirs, verdicts, &rejected, NULL);
        CHECK(st == ZIGZ_OK && rejected == 0 && verdicts[0] == 1 && verdicts[1] == 1 && verdicts[2] == 1, "verify: %d, %zu rejected", (int)st, rejected);
        st = zigz_merkle_open_batch(ctx, b, one_each, sib1, dirs1, leaves1, NULL);
        CHECK(st == ZIGZ_OK && !memcmp(sib1, sib, 96) && !memcmp(dirs1, dirs, 3) && leaves1[0] == leaves[0], "open_batch agrees");
        /* errors name the first offender and write nothing */
        {
            const uint32_t bad_trees[3] = {0, 2, 2};
            const uint64_t bad_indices[3] = {1, 5, 5};
            uint8_t keep[sizeof sib];
            memcpy(keep, sib, sizeof sib);
            st = zigz_merkle_open_many(ctx, b, 3, bad_trees, indices, sib, dirs, leaves, roots, heights, &bad);
            CHECK(st == ZIGZ_ERR_INVALID_ARGUMENT && bad == 1, "bad tree: %d at %zu", (int)st, bad);
            st = zigz_merkle_open_many(ctx, b, 3, trees, bad_indices, sib, dirs, leaves, roots, heights, &bad);
            CHECK(st == ZIGZ_ERR_INDEX_OUT_OF_BOUNDS && bad == 1, "bad index: %d at %zu", (int)st, bad);
            CHECK(!memcmp(keep, sib, sizeof sib), "outputs untouched");
        }
        zigz_merkle_batch_destroy(ctx, b);
    }
    zigz_ctx_destroy(ctx);
    if (!failures) printf("open_many_driver: ok\n");
    return failures != 0;
}
