// Prints the real bank_plan() of rmnet_amd/csrc/common.h for argument tuples read from standard input, one
// "Mq hw njt no slots" per line -> one "nqt nsplit" per line.  tests/test_memory_read_exact.py compares its Python restatement
// (tests/exact_read_ref.py) with this output.  Host code only:
//   hipcc -O1 -std=c++17 -w --offload-arch=gfx950 tests/native/bank_plan_print.cpp -o bank_plan_print
#include <cstdio>

#include "../../rmnet_amd/csrc/common.h"

int main() {
  int Mq, hw, njt, no, slots, n = 0;
  while (scanf("%d %d %d %d %d", &Mq, &hw, &njt, &no, &slots) == 5) {
    const rmnet::BankPlan p = rmnet::bank_plan(Mq, hw, njt, no, slots);
    printf("%d %d\n", p.nqt, p.nsplit);
    ++n;
  }
  fprintf(stderr, "bank_plan_print: %d tuples, kSplitMax %d, kSplitMinTiles %d, kSplitTargetSlots %d, kPlanInts %d\n", n, rmnet::kSplitMax,
          rmnet::kSplitMinTiles, rmnet::kSplitTargetSlots, rmnet::kPlanInts);
  return 0;
}
