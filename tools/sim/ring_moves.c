// Simulates one wavefront's ring protocol of the slot-code road (k_build_wave<PLANAR, CODES>, hj_build_wave.hip) on the
// CPU, chunk by chunk, to count what the ring leaves to the deferred phase under different rules for WHEN the ring moves:
//
//   rule 0  "today"  the ring moves once per tile, before the first batch, far enough for the tile's highest home slot
//   rule 1  (a)      it moves before each batch of four rows, only as far as that batch's highest home slot needs
//   rule 2  (b)      as (a), and before a move the queued entries that lie below the move's target get their rounds
//
// What is modelled: DataGen's `uniform` (srand(0), keys (rand() & (n - 1)) + 1, sorted, window shuffle W = 16), a table of
// 2n slots with the identity hash, the seams as k_wave_seams / k_wave_bounds_scan place them (look of 256 positions, head
// zone and overlap zone of 64), tiles of 512 in two batches of four rows, the home-slot attempts of a batch before its push
// rows, the FIFO retry queue with unfinished entries back to the front, a round once 64 entries wait or one per tile, the
// look over four slots inside a granule, "spent" drops, the ring-advance rule, the drain at a chunk's end. Not modelled: the
// deferred phase itself (so the few drops it finds are missing from `drops`), time, and the lanes' order inside one LDS
// instruction (lane order here; the protocol is confluent, the table does not depend on it, the counts hardly do).
//
//   cc -O2 -o ring_moves ring_moves.c
//   ring_moves LOG2N CHUNKLEN RULE PROBELEN [RING_GRANULES = 8]
//
// Prints deferred (behind the ring / seam or ahead of it), drops in the ring, rounds and forced rounds, totals and per tile.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define EMPTY 0xFFFFFFFFu
#define NONE 0xFFFFFFFFu
enum { GSH = 7, GSLOTS = 128, TILE = 512, ROWS = 4, PER = 8, LOOK = 256, OVERLAP = 64, QCAP = 128, ROUND_AT = 64 };

static uint32_t *R, *tab;            // keys by position; slot -> position of the tuple that holds it (order = position)
static uint64_t n;
static uint32_t mask, numGran, probeLen, RGRAN = 8;
static int rule;

// one wavefront's state
static uint32_t winLoG, loG, limG;
static uint32_t qPos[QCAP], qIdx[QCAP], qHead, qCount;
static uint64_t rounds, forcedRounds, forcedEntries, drops, defBehind, defSeam, tiles, moves;

static uint32_t home_of(uint32_t key) { return key & mask; }
static int in_ring(uint32_t pos) { const uint32_t g = pos >> GSH; return (uint32_t)(g - winLoG) < RGRAN && g < limG; }
static uint32_t tries_left(uint32_t idx, uint32_t pos) { return probeLen - ((pos - home_of(R[idx])) & mask); }
static void defer(uint32_t pos)
{
    const uint32_t g = pos >> GSH;
    if (g >= loG && g < winLoG) defBehind++; else defSeam++;
}

// one round on up to 64 entries held one per lane; again[] says which are not finished (their next state in place)
static void round_body(uint32_t *pos, uint32_t *idx, int cnt, int *again)
{
    int work[64], doAtomic[64];
    for (int l = 0; l < cnt; l++) {                    // the looks: every lane reads before any lane's atomic
        again[l] = 0; doAtomic[l] = 0;
        work[l] = in_ring(pos[l]);
        if (!work[l]) { defer(pos[l]); continue; }
        uint32_t skip = 0;
        if ((pos[l] & (GSLOTS - 1)) <= GSLOTS - 4)
            while (skip < 4 && tab[pos[l] + skip] < idx[l]) skip++;
        if (skip >= tries_left(idx[l], pos[l])) { drops++; continue; }       // every slot it had left holds an earlier tuple
        pos[l] = (pos[l] + skip) & mask;
        if (skip == 4) { again[l] = 1; continue; }     // may have left the granule: next round
        doAtomic[l] = 1;
    }
    for (int l = 0; l < cnt; l++) {
        if (!doAtomic[l]) continue;
        const uint32_t old = tab[pos[l]];
        if (idx[l] < old) tab[pos[l]] = idx[l];
        if (old == EMPTY || old == idx[l]) continue;   // placed
        if (old > idx[l]) idx[l] = old;                // displaced a later tuple: carry it on
        if (tries_left(idx[l], pos[l]) <= 1) { drops++; continue; }
        pos[l] = (pos[l] + 1) & mask;
        again[l] = 1;
    }
}
static void retry_round(void)
{
    const int take = qCount < 64 ? (int)qCount : 64;
    uint32_t pos[64], idx[64]; int again[64];
    for (int l = 0; l < take; l++) { pos[l] = qPos[(qHead + l) & (QCAP - 1)]; idx[l] = qIdx[(qHead + l) & (QCAP - 1)]; }
    qHead = (qHead + take) & (QCAP - 1); qCount -= take;
    round_body(pos, idx, take, again);
    int back = 0;
    for (int l = 0; l < take; l++) back += again[l];
    qHead = (qHead - back) & (QCAP - 1);
    for (int l = 0, k = 0; l < take; l++)
        if (again[l]) { qPos[(qHead + k) & (QCAP - 1)] = pos[l]; qIdx[(qHead + k) & (QCAP - 1)] = idx[l]; k++; }
    qCount += back;
    rounds++;
}
static void drain(void)
{
    while (qCount > 64) retry_round();
    uint32_t pos[64], idx[64]; int act[64], again[64], cnt = (int)qCount;
    for (int l = 0; l < cnt; l++) { pos[l] = qPos[(qHead + l) & (QCAP - 1)]; idx[l] = qIdx[(qHead + l) & (QCAP - 1)]; act[l] = 1; }
    qCount = 0;
    for (int any = cnt > 0; any;) {
        uint32_t p2[64], i2[64]; int map[64], m = 0;
        for (int l = 0; l < cnt; l++) if (act[l]) { p2[m] = pos[l]; i2[m] = idx[l]; map[m++] = l; }
        round_body(p2, i2, m, again);
        any = 0;
        for (int k = 0; k < m; k++) { pos[map[k]] = p2[k]; idx[map[k]] = i2[k]; act[map[k]] = again[k]; any |= again[k]; }
        rounds++;
    }
}
static uint32_t ring_target(uint32_t hi, uint32_t gmin)
{
    const uint32_t top = (uint32_t)(((uint64_t)hi + probeLen + 8u) >> GSH) + 1u;
    uint32_t target = top > RGRAN ? top - RGRAN : 0u;
    if (target > gmin) target = gmin;
    if (target > limG) target = limG;
    return target;
}
static void move_ring(uint32_t target)
{
    if (target <= winLoG) return;
    if (rule >= 2) {
        while (qCount >= ROUND_AT) retry_round();
        for (;;) {
            uint32_t below = 0;
            for (uint32_t l = 0; l < qCount; l++) below += qPos[(qHead + l) & (QCAP - 1)] < (target << GSH);
            if (!below) break;
            forcedRounds++; forcedEntries += qCount;
            retry_round();
        }
    }
    winLoG = target; moves++;
}

static int cmp_u32(const void *a, const void *b) { const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b; return x < y ? -1 : x > y; }
static void generate_uniform(int window)
{
    srand(0);
    for (uint64_t i = 0; i < n; i++) R[i] = ((uint32_t)rand() & (uint32_t)(n - 1)) + 1u;
    qsort(R, n, sizeof *R, cmp_u32);
    unsigned char *shuffled = calloc(n, 1);
    for (uint64_t i = 0; i + 1 < n; i++) {
        if (shuffled[i]) continue;
        const int rem = (int)(n - i), swap = rand() % (window < rem ? window : rem);
        const uint32_t t = R[i]; R[i] = R[i + swap]; R[i + swap] = t;
        shuffled[i + swap] = 1;
    }
    free(shuffled);
}

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: %s LOG2N CHUNKLEN RULE(0 today, 1 a, 2 b) PROBELEN [RING_GRANULES]\n", argv[0]); return 2; }
    n = 1ull << atoi(argv[1]);
    const uint32_t chunkLen = (uint32_t)atoi(argv[2]);
    rule = atoi(argv[3]); probeLen = (uint32_t)atoi(argv[4]);
    if (argc > 5) RGRAN = (uint32_t)atoi(argv[5]);
    if (n < 4 * TILE || n > (1ull << 30) || chunkLen < 4 * TILE || n % chunkLen || rule < 0 || rule > 2 || !probeLen || (RGRAN & (RGRAN - 1))) return 2;
    mask = (uint32_t)(2 * n - 1); numGran = (uint32_t)((2 * n) >> GSH);
    R = malloc(n * sizeof *R); tab = malloc(2 * n * sizeof *tab);
    memset(tab, 0xFF, 2 * n * sizeof *tab);
    generate_uniform(16);

    // the seams: k_wave_seams, k_wave_bounds_scan
    const uint32_t nChunks = (uint32_t)(n / chunkLen);
    uint32_t *starts = malloc((nChunks + 1) * sizeof *starts), *bounds = malloc((nChunks + 1) * sizeof *bounds);
    uint32_t run = 0;
    for (uint32_t c = 0; c < nChunks; c++) {
        const uint64_t p = (uint64_t)c * chunkLen;
        uint32_t m = NONE;
        for (uint32_t l = 0; l < 64; l++) if (home_of(R[p + l]) < m) m = home_of(R[p + l]);
        uint32_t start = (uint32_t)p, g = m >> GSH;
        if (c > 0) {
            const uint32_t edge = ((m >> GSH) + 1) << GSH;
            for (uint32_t k = 0; k < LOOK && edge; k++)
                if (home_of(R[p + k]) >= edge) { start = (uint32_t)p + k; g = edge >> GSH; break; }
        }
        starts[c] = start;
        if (g > run) run = g;
        bounds[c] = run < numGran ? run : numGran;
    }
    starts[nChunks] = (uint32_t)n; bounds[nChunks] = numGran;

    for (uint32_t c = 0; c < nChunks; c++) {
        const int last = c + 1 == nChunks;
        const uint32_t cb = starts[c], cend = starts[c + 1] - starts[c];
        const uint32_t plen = (uint32_t)(((uint64_t)cb + cend + OVERLAP < n ? (uint64_t)cb + cend + OVERLAP : n) - cb);
        loG = bounds[c]; limG = last ? numGran : bounds[c + 1];
        const uint32_t loSlot = c ? loG << GSH : 0u, limSlot = limG << GSH;
        winLoG = loG; qHead = qCount = 0;
        for (uint32_t tb = 0; tb < plen; tb += TILE, tiles++) {
            const int full = tb + TILE <= cend && tb >= OVERLAP;
            const uint64_t roundsAtTileStart = rounds;
            int live[TILE]; uint32_t home[TILE];
            uint32_t tmin = NONE, tmax = 0, tmaxA = 0;
            for (uint32_t o = 0; o < TILE; o++) {                     // row j = o / 64, lane = o % 64
                const uint32_t at = tb + o;
                const uint32_t key = at < plen ? R[cb + at] : 0u;
                home[o] = home_of(key);
                const int mine = full || (at < cend ? !(at < OVERLAP && home[o] < loSlot) : (at < plen && !last && home[o] < limSlot));
                live[o] = mine && key != 0;
                if (full || live[o]) {
                    if (home[o] < tmin) tmin = home[o];
                    if (home[o] > tmax) tmax = home[o];
                    if (o < 64 * ROWS && home[o] > tmaxA) tmaxA = home[o];
                }
            }
            if (tmin == NONE) continue;
            const uint32_t gmin = tmin >> GSH;
            for (int b = 0; b < PER; b += ROWS) {
                if (b == 0) move_ring(ring_target(rule == 0 ? tmax : tmaxA, gmin));
                else if (rule != 0) move_ring(ring_target(tmax, gmin));
                uint32_t old[64 * ROWS]; int own[64 * ROWS];
                for (uint32_t o = 0; o < 64 * ROWS; o++) {            // the batch's home-slot attempts, issued together
                    const uint32_t t = 64 * b + o, idx = cb + tb + t;
                    own[o] = live[t] && in_ring(home[t]);
                    old[o] = EMPTY;
                    if (own[o]) { old[o] = tab[home[t]]; if (idx < old[o]) tab[home[t]] = idx; }
                }
                for (int r = 0; r < ROWS; r++) {                      // the push rows
                    while (qCount >= ROUND_AT) retry_round();
                    for (uint32_t l = 0; l < 64; l++) {
                        const uint32_t o = 64 * r + l, t = 64 * b + o;
                        uint32_t idx = cb + tb + t, pos = home[t];
                        int again = live[t] && !own[o];               // outside ring or range: the retry round defers it
                        if (own[o] && old[o] != EMPTY) {
                            if (old[o] > idx) idx = old[o];
                            if (tries_left(idx, pos) <= 1) drops++;
                            else { pos = (pos + 1) & mask; again = 1; }
                        }
                        if (again) { qPos[(qHead + qCount) & (QCAP - 1)] = pos; qIdx[(qHead + qCount) & (QCAP - 1)] = idx; qCount++; }
                    }
                }
            }
            while (qCount >= ROUND_AT) retry_round();
            if (qCount && rounds == roundsAtTileStart) retry_round();
        }
        if (qCount) drain();
    }
    uint64_t placed = 0;
    for (uint64_t s = 0; s < 2 * n; s++) placed += tab[s] != EMPTY;
    const double t = (double)tiles;
    printf("log2n %s chunk %u rule %d probeLength %u ring %u granules: chunks %u tiles %llu\n", argv[1], chunkLen, rule, probeLen, RGRAN, nChunks,
           (unsigned long long)tiles);
    printf("deferred %llu (behind the ring %llu, seam or ahead %llu) = %.4f %% of R\n", (unsigned long long)(defBehind + defSeam),
           (unsigned long long)defBehind, (unsigned long long)defSeam, 100.0 * (double)(defBehind + defSeam) / (double)n);
    printf("drops in the ring %llu = %.2f %% of R; placed in the ring %llu\n", (unsigned long long)drops, 100.0 * (double)drops / (double)n,
           (unsigned long long)placed);
    printf("rounds %llu = %.3f per tile; forced rounds %llu = %.3f per tile, %.1f entries each; ring moves %.2f per tile\n",
           (unsigned long long)rounds, (double)rounds / t, (unsigned long long)forcedRounds, (double)forcedRounds / t,
           forcedRounds ? (double)forcedEntries / (double)forcedRounds : 0.0, (double)moves / t);
    return 0;
}
