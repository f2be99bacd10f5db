#!/bin/bash
# CPU-side sanitizer pass (GPU ASan is not available on this pool): the oracle and the product's host-side
# DataGen under -fsanitize=address,undefined, exercised through small C/C++ drivers.
set -e
cd "$(dirname "$0")/.."
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
cat > $T/san_oracle.c <<'C'
#include "hj_oracle.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(void) {
    const char *dists[] = {"uniform", "random", "sorted", "shuffle", "local_shuffle"};
    for (int d = 0; d < 5; d++) for (uint64_t n = 1; n <= (1u << 14); n = n * 4 + 1) {
        uint64_t np2 = 1; while (np2 < n) np2 <<= 1;
        uint64_t *R = malloc(np2 * 8), *S = malloc((np2 + 3) * 8), *T = malloc(2 * np2 * 8);
        orc_generate_data(dists[d], np2, np2, 16, R);
        orc_generate_data("sorted", np2, np2, 16, S); S[np2] = 1; S[np2 + 1] = 2 * np2 - 1; S[np2 + 2] = 4 * np2 - 1;
        orc_result r, m; orc_prj_result p;
        orc_build_probe_seq(R, np2, S, np2 + 3, 4, &r, T);
        orc_build_probe_seq_ts(R, np2, S, np2 + 3, 3, 2 * np2, 1, &r, T);
        orc_build_probe_mt(R, np2, S, np2 + 3, 4, 64 < np2 ? 64 : 1, 4, 0, &m);
        orc_build_probe_mt(R, np2, S, np2 + 3, 4, 64 < np2 ? 64 : 1, 4, 1, &m);
        orc_prj_join(R, np2, S, np2 + 3, np2 > 64 ? 7 : 2, &p);
        if (p.matches != orc_true_cardinality(R, np2, S, np2 + 3)) { printf("PRJ mismatch\n"); return 1; }
        free(R); free(S); free(T);
    }
    uint64_t z[1000]; orc_generate_zipf(1000, 64, 0.9, 1, z);
    printf("oracle sanitizer pass ok\n");
    return 0;
}
C
gcc -O1 -g -std=gnu99 -fsanitize=address,undefined -fno-omit-frame-pointer -Ioracle $T/san_oracle.c oracle/hj_oracle.c -o $T/san_oracle -lpthread -lm
$T/san_oracle
cat > $T/san_datagen.cpp <<'C'
#include "include/htm_hashjoin.h"
#include <cstdio>
#include <vector>
int main() {
    const char* dists[] = {"uniform", "random", "sorted", "shuffle", "local_shuffle", "zipf"};
    for (const char* d : dists) for (uint64_t n : {1ull, 2ull, 1000ull, 70000ull, 300000ull}) {
        std::vector<uint64_t> v(n);
        if (hj_generate_data(d, n, n > 1 ? n : 2, 16, 0.9, v.data()) != HJ_OK) { printf("fail %s\n", d); return 1; }
    }
    std::vector<uint64_t> v(8);
    if (hj_generate_data("nope", 8, 8, 16, 0, v.data()) != HJ_ERR_INVALID) return 1;
    printf("datagen sanitizer pass ok\n");
    return 0;
}
C
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -I. $T/san_datagen.cpp htm-hashjoin_amd/csrc/hj_datagen.cpp -o $T/san_datagen -lpthread
$T/san_datagen
