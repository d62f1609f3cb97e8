// The host check of the command areas' inputs (elmkernels_amd/csrc/elmk_maps.h: command_check), case by case: prints
// "<case>: <returned text>", or for accepted inputs "<case>: ok" followed, where asked for, by the dam list, ptr and the terms as
// "cell/slot/share" with the share a hexadecimal double.  tests/test_routing_command_host.py compares every line with the message
// elmk_routing_command_enable gives behind its own name and the tables with routing.command_tables, bit for bit.
#include "elmk_maps.h"

#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace elmk;

namespace {
const double NaN = std::numeric_limits<double>::quiet_NaN();
const double Inf = std::numeric_limits<double>::infinity();

struct Inputs {
  std::vector<double> cap, share, claim;
  std::vector<int32_t> dam;
  void set(int64_t n, int k, int64_t c, int32_t d, double s, double q)
  {
    dam[(size_t)k * (size_t)n + (size_t)c] = d;
    share[(size_t)k * (size_t)n + (size_t)c] = s;
    claim[(size_t)k * (size_t)n + (size_t)c] = q;
  }
};

// n >= 12 cells, dams in cells 2, 5 (of the smallest capacity) and 9 (without dependents); cell 0 hangs on 2 and 5, cell 1 on 5, the dam
// cell 5 on 2, cell 7 on 5 and 2 in that order; empty slots hold what must not be read
Inputs valid(int64_t n)
{
  Inputs in;
  in.cap.assign((size_t)n, 0.0);
  in.cap[2] = 1.0e9;
  in.cap[5] = 5e-324;
  in.cap[9] = 3.0e7;
  in.dam.assign((size_t)COMMAND_NDEP * (size_t)n, -1);
  in.share.assign((size_t)COMMAND_NDEP * (size_t)n, NaN);
  in.claim.assign((size_t)COMMAND_NDEP * (size_t)n, -7.0);
  in.set(n, 0, 0, 2, 0.5, 0.25);
  in.set(n, 1, 0, 5, 0.5, 1.0);
  in.set(n, 0, 1, 5, 1.0, 0.0);
  in.set(n, 0, 5, 2, 0.125, 0.25);
  in.set(n, 0, 7, 5, 0.375, 0.0);
  in.set(n, 1, 7, 2, 0.0625, 0.5);
  return in;
}

void say(const std::string& name, int64_t n, const Inputs& in, bool show = false)
{
  const int64_t ld = (n + 63) / 64 * 64;
  CommandTables T;
  int64_t cell = -1;
  const char* const text = command_check(n, in.cap.data(), in.dam.data(), in.share.data(), in.claim.data(), ld, &T, &cell);
  if (text) {
    if (cell >= 0) printf("%s: %s at cell %lld\n", name.c_str(), text, (long long)cell);
    else printf("%s: %s\n", name.c_str(), text);
    return;
  }
  std::string s;
  const size_t l = (size_t)ld;
  if (T.dam.size() != COMMAND_NDEP * l || T.share.size() != COMMAND_NDEP * l || T.claim.size() != COMMAND_NDEP * l) s = " BAD SIZE";
  for (int k = 0; k < COMMAND_NDEP && s.empty(); k++)
    for (size_t c = (size_t)n; c < l; c++)
      if (T.dam[(size_t)k * l + c] != -1 || T.share[(size_t)k * l + c] != 0.0 || T.claim[(size_t)k * l + c] != 0.0) s = " BAD PADDING CELL";
  for (int k = 0; k < COMMAND_NDEP && s.empty(); k++)
    for (size_t c = 0; c < (size_t)n; c++)
      if (T.dam[(size_t)k * l + c] < 0 && (T.share[(size_t)k * l + c] != 0.0 || T.claim[(size_t)k * l + c] != 0.0)) s = " BAD EMPTY SLOT";
  if (T.ptr.size() != T.dams.size() + 1 || T.tcell.size() != (size_t)T.ptr.back() || T.tshare.size() != T.tcell.size()) s = " BAD MAP";
  printf("%s: ok%s", name.c_str(), s.c_str());
  if (show && s.empty()) {
    printf(" dams");
    for (int32_t d : T.dams) printf(" %d", (int)d);
    printf(" ptr");
    for (int64_t p : T.ptr) printf(" %lld", (long long)p);
    printf(" terms");
    for (size_t p = 0; p < T.tcell.size(); p++) printf(" %d/%d/%a", (int)T.tcell[p], (int)T.tslot[p], T.tshare[p]);
  }
  printf("\n");
}
}  // namespace

int main()
{
  const int64_t n = 12;
  const Inputs good = valid(n);
  {
    int64_t cell = 5;
    const char* t = command_check(0, good.cap.data(), good.dam.data(), good.share.data(), good.claim.data(), 64, nullptr, &cell);
    printf("ncells 0: %s %lld\n", t ? t : "", (long long)cell);
    t = command_check(n, nullptr, good.dam.data(), good.share.data(), good.claim.data(), 64, nullptr, nullptr);
    printf("null cap: %s\n", t ? t : "");
    t = command_check(n, good.cap.data(), nullptr, good.share.data(), good.claim.data(), 64, nullptr, nullptr);
    printf("null dam: %s\n", t ? t : "");
    t = command_check(n, good.cap.data(), good.dam.data(), nullptr, good.claim.data(), 64, nullptr, nullptr);
    printf("null share: %s\n", t ? t : "");
    t = command_check(n, good.cap.data(), good.dam.data(), good.share.data(), nullptr, 64, nullptr, nullptr);
    printf("null claim: %s\n", t ? t : "");
  }
  const int32_t bad_index[] = {-2, 12, INT32_MAX, INT32_MIN};
  for (int b = 0; b < 4; b++) {
    Inputs in = good;
    in.dam[(size_t)1 * (size_t)n + 1] = bad_index[b];  // (an index out of range is refused wherever it stands, behind an empty slot too)
    say("bad index " + std::to_string(b), n, in);
  }
  {
    Inputs in = good;
    in.set(n, 2, 1, 2, 0.5, 0.0);  // slot 1 of cell 1 is empty
    say("gap", n, in);
    in = good;
    in.set(n, 1, 1, 3, 0.5, 0.0);
    say("no reservoir", n, in);
    in = good;
    in.set(n, 1, 5, 5, 0.5, 0.0);
    say("itself", n, in);
    in = good;
    in.set(n, 2, 7, 5, 0.25, 0.0);
    say("twice", n, in);
  }
  const double bad_share[] = {0.0, -0.5, 1.0000000000000002, NaN, Inf};
  for (int b = 0; b < 5; b++) {
    Inputs in = good;
    in.share[(size_t)1 * (size_t)n + 7] = bad_share[b];
    say("bad SHARE " + std::to_string(b), n, in);
  }
  const double bad_claim[] = {-1.0e-9, 1.0000000000000002, NaN, Inf};
  for (int b = 0; b < 4; b++) {
    Inputs in = good;
    in.claim[(size_t)0 * (size_t)n + 5] = bad_claim[b];
    say("bad CLAIM " + std::to_string(b), n, in);
  }
  {
    Inputs in = good;
    in.share[(size_t)1 * (size_t)n + 0] = 0.5000000000000002;
    say("shares above 1", n, in);
    in = good;
    in.claim[(size_t)1 * (size_t)n + 7] = 0.5000000000000002;  // dam 2: 0.25 + 0.25 + this
    say("claims above 1", n, in);
    in.share[(size_t)0 * (size_t)n + 1] = 2.0;  // violated twice: the cells' rows are checked before any dam's claims
    say("cells before dams", n, in);
    in = good;
    in.share[(size_t)0 * (size_t)n + 7] = 0.0;  // two cells violated: the first cell is named
    in.share[(size_t)0 * (size_t)n + 1] = NaN;
    say("first cell", n, in);
  }
  say("valid", n, good, true);
  {
    Inputs in = valid(65);
    in.set(65, 0, 64, 9, 1.0, 1.0);
    say("sixty-five cells", 65, in, true);
    Inputs none = valid(n);
    none.dam.assign(none.dam.size(), -1);
    say("no dependents", n, none, true);
    none.cap.assign((size_t)n, 0.0);
    say("no dams", n, none, true);
  }
  return 0;
}
