// Host check of the slot arithmetic of the LDS Verlet lists (neuralmelting_amd/csrc/nm_math.h: list_slot, list_slot_shifted), the text the
// kernels compile.  Reads lines "lt lpw nlist maxnb" (log2 of the threads per row, log2 of the entries per 8-byte word, rows per list, entries
// per row) and, for each, walks every rank rr < maxnb the way Replica::rebuild's append loop does — from every starting rank, rp = rr << lpw
// counted up by 2^lpw — and compares list_slot_shifted(rp) with list_slot(rr) and with the reader's expression written out here (nbr_at:
// sub = rr % TPA, k = rr / TPA, element (((k / PW) * NLIST + row) * TPA + sub) * PW + k % PW) for the first and the last row.  Also that the
// slots of a row are distinct and stay inside the list.  Prints "ok <cases>" per line, or the first mismatch and exits 1.
#include <cstdio>
#include <vector>
#define NM_HD
#include "nm_math.h"

int main()
{
    unsigned int lt, lpw, nlist, maxnb;
    while (std::scanf("%u %u %u %u", &lt, &lpw, &nlist, &maxnb) == 4) {
        const unsigned int tpa = 1u << lt, pw = 1u << lpw, chunk = nlist * tpa * pw, total = maxnb * nlist;
        unsigned long long cases = 0;
        std::vector<char> seen(total);
        for (unsigned int row : { 0u, nlist - 1u }) {
            const unsigned int rowc = (row * tpa) << lpw;
            std::fill(seen.begin(), seen.end(), 0);
            for (unsigned int rr = 0; rr < maxnb; ++rr) {
                const unsigned int sub = rr % tpa, k = rr / tpa;
                const unsigned int reader = (((k / pw) * nlist + row) * tpa + sub) * pw + k % pw;
                const unsigned int now = rowc + nm::list_slot(rr, lt, lpw, chunk);
                if (now != reader || now >= total || seen[now]) { std::printf("list_slot: lt %u lpw %u nlist %u row %u rr %u: %u, reader %u\n", lt, lpw, nlist, row, rr, now, reader); return 1; }
                seen[now] = 1;
            }
            for (unsigned int r0 = 0; r0 < maxnb; ++r0) { // a thread's first rank; it appends at most 32 entries
                unsigned int rp = r0 << lpw;
                for (unsigned int rr = r0; rr < maxnb && rr < r0 + 32u; ++rr, rp += pw, ++cases) {
                    const unsigned int want = rowc + nm::list_slot(rr, lt, lpw, chunk), got = rowc + nm::list_slot_shifted(rp, lt, lpw, chunk);
                    if (got != want) { std::printf("list_slot_shifted: lt %u lpw %u nlist %u row %u from %u rr %u: %u, want %u\n", lt, lpw, nlist, row, r0, rr, got, want); return 1; }
                }
            }
        }
        std::printf("ok %llu\n", cases);
    }
    return 0;
}
