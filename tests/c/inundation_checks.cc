// The host check of the floodplain inundation's inputs (elmkernels_amd/csrc/elmk_maps.h: inundation_check), case by case: prints
// "<case>: <returned text>", or for accepted inputs "<case>: ok" followed by the 25 table rows of every cell as hexadecimal doubles
// and the state of the padding cells.  tests/test_routing_inundation_host.py compares every line with the message
// elmk_routing_inundation_enable gives behind its own name and the tables with routing.inundation_tables, bit for bit.  Built with
// -ffp-contract=off, as the library is: I0 has products under sums.
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
  std::vector<double> rdepth, eprof, area, rlen, rwidth;
};

// cells that share no quotient: banks of 0.5 m and up, profile steps that grow with k, a cell of no area (the second) and one whose
// channel is wider than its cell (the third) where there are cells enough
Inputs valid(int64_t n)
{
  Inputs in;
  for (int64_t c = 0; c < n; c++) {
    in.rdepth.push_back(0.5 + 0.37 * (double)(c % 7));
    in.area.push_back(c == 1 ? 0.0 : 1.0e8 * (1.0 + 0.011 * (double)(c % 13)));
    in.rlen.push_back(2.0e4 * (1.0 + 0.013 * (double)((c * 7) % 11)));
    in.rwidth.push_back(c == 2 ? 1.0e4 : 100.0 * (1.0 + 0.017 * (double)((c * 3) % 5)));
  }
  in.eprof.assign((size_t)INUNDATION_NPROF * (size_t)n, 0.0);
  for (int k = 1; k < INUNDATION_NPROF; k++)
    for (int64_t c = 0; c < n; c++)
      in.eprof[(size_t)k * (size_t)n + (size_t)c] = in.eprof[(size_t)(k - 1) * (size_t)n + (size_t)c] + 0.013 * (double)(k + c % 3) + 0.001;
  return in;
}

// the text as the entry point forms it: " at cell <cell>" behind it where the check names a cell
std::string check(int64_t n, const double* rdepth, const double* eprof, const double* area, const double* rlen, const double* rwidth,
                  int64_t ld, std::vector<double>* dev)
{
  int64_t cell = -1;
  const char* const text = inundation_check(n, rdepth, eprof, area, rlen, rwidth, ld, dev, &cell);
  if (!text) return std::string();
  return cell >= 0 ? std::string(text) + " at cell " + std::to_string(cell) : std::string(text);
}

void say(const std::string& name, int64_t n, const Inputs& in, bool show = false)
{
  const int64_t ld = (n + 63) / 64 * 64;
  std::vector<double> dev;
  const std::string text = check(n, in.rdepth.data(), in.eprof.data(), in.area.data(), in.rlen.data(), in.rwidth.data(), ld, &dev);
  if (!text.empty()) {
    printf("%s: %s\n", name.c_str(), text.c_str());
    return;
  }
  std::string s;
  if (dev.size() != (size_t)25 * (size_t)ld) s = " BAD SIZE";
  for (int k = 0; k < 25 && s.empty(); k++)
    for (int64_t c = n; c < ld; c++)
      if (dev[(size_t)k * (size_t)ld + (size_t)c] != 0.0) s = " BAD PADDING CELL";
  printf("%s: ok%s", name.c_str(), s.c_str());
  if (show && s.empty())
    for (int k = 0; k < 25; k++)
      for (int64_t c = 0; c < n; c++) printf(" %a", dev[(size_t)k * (size_t)ld + (size_t)c]);
  printf("\n");
}
}  // namespace

int main()
{
  const int64_t n = 5;
  const Inputs good = valid(n);
  const auto run = [&](int64_t cells, const double* rdepth, const double* eprof) {
    return check(cells, rdepth, eprof, nullptr, nullptr, nullptr, 64, nullptr);
  };
  printf("ncells 0: %s\n", run(0, good.rdepth.data(), good.eprof.data()).c_str());
  printf("ncells 2^31: %s\n", run((int64_t)1 << 31, good.rdepth.data(), good.eprof.data()).c_str());
  printf("null rdepth: %s\n", run(n, nullptr, good.eprof.data()).c_str());
  printf("null eprof: %s\n", run(n, good.rdepth.data(), nullptr).c_str());
  {
    std::vector<double> dev;  // tables asked for without the cells' geometry
    printf("null area: %s\n", check(n, good.rdepth.data(), good.eprof.data(), nullptr, good.rlen.data(), good.rwidth.data(), 64, &dev).c_str());
  }
  const double bads[] = {0.0, -0.0, -1.0, NaN, Inf, -Inf};
  const char* const bad_names[] = {"0", "-0", "negative", "NaN", "inf", "-inf"};
  for (int b = 0; b < 6; b++) {
    Inputs in = good;
    in.rdepth[(size_t)(b % n)] = bads[b];  // (first, middle and last cells in turn)
    say(std::string("RDEPTH ") + bad_names[b], n, in);
  }
  for (int k = 0; k < INUNDATION_NPROF; k++)
    for (int b = 3; b < 6; b++) {
      Inputs in = good;
      in.eprof[(size_t)k * (size_t)n + (size_t)((k + b) % n)] = bads[b];
      say("EPROF[" + std::to_string(k) + "] " + bad_names[b], n, in);
    }
  {
    Inputs in = good;
    in.eprof[3] = 1.0e-3;  // cell 3 starts above the bank top
    say("EPROF[0] positive", n, in);
    in = good;
    in.eprof[3] = -1.0e-3;
    say("EPROF[0] negative", n, in);
    in = good;
    in.eprof[3] = -0.0;  // -0.0 == 0.0: accepted
    say("EPROF[0] -0", n, in);
  }
  for (int k = 1; k < INUNDATION_NPROF; k++) {
    Inputs in = good;
    const size_t c = (size_t)(k % n);
    in.eprof[(size_t)k * (size_t)n + c] = in.eprof[(size_t)(k - 1) * (size_t)n + c];  // a flat step
    say("EPROF[" + std::to_string(k) + "] flat", n, in);
    in.eprof[(size_t)k * (size_t)n + c] = in.eprof[(size_t)(k - 1) * (size_t)n + c] - 0.5;  // a falling one
    say("EPROF[" + std::to_string(k) + "] falling", n, in);
  }
  {
    Inputs in = good;  // two cells violated at once: the profile is checked cell by cell, rdepth before any of it
    in.eprof[(size_t)5 * (size_t)n + 4] = NaN;
    in.eprof[(size_t)9 * (size_t)n + 2] = 0.0;
    say("falling in cell 2 and NaN in cell 4", n, in);
    in.rdepth[4] = 0.0;
    say("... and bad RDEPTH in cell 4", n, in);
  }
  {
    Inputs in = good;  // denormal and huge values are finite and > 0
    in.rdepth[0] = 5e-324;
    in.eprof[(size_t)10 * (size_t)n + 1] = 1.7e308;
    say("denormal RDEPTH and huge EPROF[10]", n, in);
  }
  say("valid", n, good, true);
  say("one cell", 1, valid(1), true);
  say("sixty-four cells", 64, valid(64));
  say("sixty-five cells", 65, valid(65));
  {
    std::vector<double> dev;  // ld below ncells: the rows are as long as the cells
    const std::string text = check(n, good.rdepth.data(), good.eprof.data(), good.area.data(), good.rlen.data(), good.rwidth.data(), 0, &dev);
    printf("ld 0: %s size=%zu\n", text.empty() ? "ok" : text.c_str(), dev.size());
  }
  return 0;
}
