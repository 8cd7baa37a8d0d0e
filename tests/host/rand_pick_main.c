/* sparc_rand_pick of include/sparc_gym_amd.h on the triples of a file (test_rand_pick.py):
 * argv[1] holds n records of three little-endian u64 (seed, id, t); argv[2] receives, for each of
 * the 16 masks, n bytes: the pick. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "sparc_gym_amd.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    fseek(in, 0, SEEK_END);
    const long n = ftell(in) / 24;
    fseek(in, 0, SEEK_SET);
    uint64_t *v = malloc((size_t)n * 24);
    if (!v || fread(v, 24, (size_t)n, in) != (size_t)n) return 4;
    for (uint32_t mask = 0; mask < 16; ++mask)
        for (long i = 0; i < n; ++i) fputc((int)sparc_rand_pick(v[3 * i], v[3 * i + 1], v[3 * i + 2], mask), out);
    free(v);
    fclose(in);
    return fclose(out) ? 5 : 0;
}
