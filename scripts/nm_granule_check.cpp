// Host check of the hand-over granule's predicate (neuralmelting_amd/csrc/nm_math.h: granule_state), the text the kernels compile:
// reads words x = word0 ^ word1 ^ magic in hexadecimal, one per line, and prints 0 (invalid), 1 (valid) or 2 (valid and poisoned)
// for each.  tests/test_granule_check.py chooses the words and knows the answers.
#include <cstdio>
#define NM_HD
#include "nm_math.h"

int main()
{
    unsigned long long x;
    std::printf("poison %llx\n", nm::GRANULE_POISON);
    while (std::scanf("%llx", &x) == 1) {
        const nm::GranuleState s = nm::granule_state(x);
        if (s.poisoned && !s.valid) { std::printf("poisoned but not valid: %llx\n", x); return 1; }
        std::printf("%d\n", s.valid ? (s.poisoned ? 2 : 1) : 0);
    }
    return 0;
}
