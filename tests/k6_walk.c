// TEST INFRASTRUCTURE: the band walk of tests/k6_cases.py (alignment specification v1, rule 7, one side) for halves of tens of
// thousands of rows, where the numpy walk takes too long.  Written from the rule's text with two rolling rows; it shares no
// code with the oracle, the engine or tests/spec_v1.py, and tests/test_host_k6_edges.py holds it to the numpy walk, row by row.
// A, B: base codes 0..3 = ACGT, 4 = anything else, in walking order (rows consume A, columns consume B).
// out[0..2] = score, row, column of the first best cell; lo / hi / best hold lenA + 1 entries: first and last live column of
// every row and the best score once the row is done.  Returns the last live row.
#include <stdint.h>
#include <stdlib.h>

static const int SUB[5][5] = {{91, -114, -31, -123, -100}, {-114, 100, -125, -31, -100}, {-31, -125, 100, -114, -100},
                              {-123, -31, -114, 91, -100}, {-100, -100, -100, -100, -100}};
#define DEAD (-((int64_t)1 << 50))
#define LIVE(x) ((x) > DEAD / 2)

int64_t k6_walk(const uint8_t *A, uint32_t lenA, const uint8_t *B, uint32_t lenB, int32_t O, int32_t E, int32_t Y, int64_t *out,
                uint32_t *lo_out, uint32_t *hi_out, int64_t *best_out) {
    int64_t *mem = malloc(((size_t)lenB + 2) * 4 * sizeof(int64_t)), *C = mem;
    if (!mem) return -1;
    int64_t *D = C + lenB + 2, *C1 = D + lenB + 2, *D1 = C1 + lenB + 2;
    uint32_t lo = 0, hi = 0;
    if (Y >= O + E) hi = (uint32_t)((Y - O) / E) < lenB ? (uint32_t)((Y - O) / E) : lenB;
    for (uint32_t j = 0; j <= hi; j++) { C[j] = j ? -(int64_t)O - (int64_t)j * E : 0; D[j] = DEAD; }
    int64_t bs = 0;
    uint32_t bi = 0, bj = 0, last = 0;
    lo_out[0] = 0; hi_out[0] = hi; best_out[0] = 0;
    for (uint32_t i = 1; i <= lenA; i++) {
        const int64_t thr = bs - Y;
        const int a = A[i - 1];
        int64_t ins = DEAD, rb = DEAD;   // the column gap arriving at column j
        uint32_t first = 0, lastj = 0, rj = 0;
        int any = 0;
        for (uint32_t j = lo; j <= lenB; j++) {
            const int in = j <= hi;
            if (!in && j > hi + 1 && !(LIVE(ins) && ins >= thr)) break;   // beyond hi + 1 only the column gap feeds a cell
            int64_t d = DEAD, g = DEAD;
            if (in && LIVE(D[j])) d = D[j] - E;
            if (in && LIVE(C[j]) && C[j] - O - E > d) d = C[j] - O - E;
            if (j >= 1 && j - 1 >= lo && j - 1 <= hi && LIVE(C[j - 1])) g = C[j - 1] + SUB[a][B[j - 1]];
            const int64_t h = d > g ? d : g;
            int64_t c = ins > h ? ins : h;
            if (LIVE(c) && c >= thr) {
                if (!any) first = j;
                any = 1; lastj = j;
                if (c > rb) { rb = c; rj = j; }
                C1[j] = c; D1[j] = d;
            } else { C1[j] = DEAD; D1[j] = DEAD; }
            int64_t ni = LIVE(ins) ? ins - E : DEAD;
            if (LIVE(h) && h - O - E > ni) ni = h - O - E;   // from the cell's H, pruned or not
            ins = ni;
        }
        if (!any) break;
        lo = first; hi = lastj; last = i;
        if (rb > bs) { bs = rb; bi = i; bj = rj; }
        lo_out[i] = lo; hi_out[i] = hi; best_out[i] = bs;
        int64_t *t = C; C = C1; C1 = t;
        t = D; D = D1; D1 = t;
    }
    out[0] = bs; out[1] = bi; out[2] = bj;
    free(mem);
    return (int64_t)last;
}
