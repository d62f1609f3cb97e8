// The host check of the reservoirs' inputs (elmkernels_amd/csrc/elmk_maps.h: reservoir_check) and their calendar, case by case:
// prints "<case>: <returned text>", or for accepted inputs "<case>: ok" followed, where asked for, by the 16 table rows of every cell as
// hexadecimal doubles and MSTART.  tests/test_routing_reservoir_host.py compares every line with the message
// elmk_routing_reservoir_enable gives behind its own name and the tables with routing.reservoir_tables, bit for bit.
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
  std::vector<double> cap, target, beta;
  std::vector<int32_t> mstart;
};

// five cells: no dam, a dam, a dam of the smallest capacity, a dam, no dam; the cells without a dam hold what must not be read
Inputs valid(int64_t n)
{
  Inputs in;
  const double caps[5] = {0.0, 2.0e9, 5e-324, 7.5e8, 0.0};
  const double betas[5] = {9.0, 0.25, 1.0, 0.0, -1.0};
  const int32_t ms[5] = {40, 11, 0, 5, -2};
  for (int64_t c = 0; c < n; c++) {
    in.cap.push_back(caps[c % 5]);
    in.beta.push_back(betas[c % 5]);
    in.mstart.push_back(ms[c % 5]);
  }
  for (int m = 0; m < RESERVOIR_NMONTH; m++)
    for (int64_t c = 0; c < n; c++) in.target.push_back(10.0 * (double)(m + 1) + (double)c);
  return in;
}

std::string check(int64_t n, const double* cap, const double* target, const double* beta, const int32_t* mstart, int64_t ld,
                  std::vector<double>* dev, std::vector<int32_t>* mdev)
{
  int64_t cell = -1;
  const char* const text = reservoir_check(n, cap, target, beta, mstart, ld, dev, mdev, &cell);
  if (!text) return std::string();
  return cell >= 0 ? std::string(text) + " at cell " + std::to_string(cell) : std::string(text);
}

void say(const std::string& name, int64_t n, const Inputs& in, bool show = false)
{
  const int64_t ld = (n + 63) / 64 * 64;
  std::vector<double> dev;
  std::vector<int32_t> mdev;
  const std::string text = check(n, in.cap.data(), in.target.data(), in.beta.data(), in.mstart.data(), ld, &dev, &mdev);
  if (!text.empty()) {
    printf("%s: %s\n", name.c_str(), text.c_str());
    return;
  }
  std::string s;
  if (dev.size() != (size_t)RESERVOIR_NTAB * (size_t)ld || mdev.size() != (size_t)ld) s = " BAD SIZE";
  for (int k = 0; k < RESERVOIR_NTAB && s.empty(); k++)
    for (int64_t c = n; c < ld; c++)
      if (dev[(size_t)k * (size_t)ld + (size_t)c] != 0.0 || mdev[(size_t)c] != 0) s = " BAD PADDING CELL";
  printf("%s: ok%s", name.c_str(), s.c_str());
  if (show && s.empty()) {
    for (int k = 0; k < RESERVOIR_NTAB; k++)
      for (int64_t c = 0; c < n; c++) printf(" %a", dev[(size_t)k * (size_t)ld + (size_t)c]);
    for (int64_t c = 0; c < n; c++) printf(" %d", (int)mdev[(size_t)c]);
  }
  printf("\n");
}
}  // namespace

int main()
{
  const int64_t n = 5;
  const Inputs good = valid(n);
  const auto run = [&](int64_t cells, const double* cap, const double* target, const double* beta, const int32_t* mstart) {
    return check(cells, cap, target, beta, mstart, 64, nullptr, nullptr);
  };
  printf("ncells 0: %s\n", run(0, good.cap.data(), good.target.data(), good.beta.data(), good.mstart.data()).c_str());
  printf("null cap: %s\n", run(n, nullptr, good.target.data(), good.beta.data(), good.mstart.data()).c_str());
  printf("null target: %s\n", run(n, good.cap.data(), nullptr, good.beta.data(), good.mstart.data()).c_str());
  printf("null beta: %s\n", run(n, good.cap.data(), good.target.data(), nullptr, good.mstart.data()).c_str());
  printf("null mstart: %s\n", run(n, good.cap.data(), good.target.data(), good.beta.data(), nullptr).c_str());
  const double bad_cap[] = {-1.0, NaN, Inf, -Inf};
  for (int b = 0; b < 4; b++) {
    Inputs in = good;
    in.cap[(size_t)b] = bad_cap[b];
    say("bad CAP " + std::to_string(b), n, in);
  }
  const double bad_target[] = {-1.0e-3, NaN, Inf};
  for (int b = 0; b < 3; b++) {
    Inputs in = good;
    const size_t c = (size_t)(b + 1);  // the three dam cells
    in.target[(size_t)(4 * b) * (size_t)n + c] = bad_target[b];
    say("bad TARGET " + std::to_string(c), n, in);
  }
  const double bad_beta[] = {-1.0e-9, 1.0000000001, NaN};
  for (int b = 0; b < 3; b++) {
    Inputs in = good;
    in.beta[(size_t)(b + 1)] = bad_beta[b];
    say("bad BETA " + std::to_string(b + 1), n, in);
  }
  const int32_t bad_ms[] = {-1, 12, INT32_MIN};
  for (int b = 0; b < 3; b++) {
    Inputs in = good;
    in.mstart[(size_t)(b + 1)] = bad_ms[b];
    say("bad MSTART " + std::to_string(b + 1), n, in);
  }
  {
    Inputs in = good;  // the rows of a cell without a dam are not read, whatever they hold
    in.target[0] = NaN;
    in.target[(size_t)11 * (size_t)n + 4] = -Inf;
    in.beta[0] = NaN;
    in.mstart[4] = INT32_MAX;
    in.cap[4] = -0.0;
    say("no dam holds anything", n, in);
    in.beta[1] = 2.0;  // violated twice: cap is checked before any other row
    in.cap[4] = -1.0;
    say("cap before the rest", n, in);
  }
  say("valid", n, good, true);
  say("sixty-five cells", 65, valid(65));
  printf("months:");
  for (int64_t d = -1; d <= 365; d++) printf(" %d", reservoir_month(d));
  printf("\nbegins:");
  for (int64_t d = -1; d <= 365; d++)
    if (reservoir_month_begins(d, (double)d + 1.0)) printf(" %d", (int)d);
  printf("\nbegins off the hour: %d\n", (int)reservoir_month_begins(31, 32.0 + 1800.0 / 86400.0));
  return 0;
}
