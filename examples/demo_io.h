// demo_io.h - the input file of the examples above include/elmk_interface.hpp, read once: the library has no file readers, and the
// demos have none of their own either.  The tests write the file (tests/support.py::state_blob).
//
// state.bin: int64 ncols; then records until EOF: char name[32]; int32 kind (0 field [column][level], 1 parameter block);
//            int64 nbytes; payload.
// Parameter blocks every file has: "land" (int32 ltype, ctype, vtype, urbpoi, lakpoi), "scalars" (dewmx, oldfflag, dayl, max_dayl,
// dt), the PFT and soil colour tables, "snicar/<i>" (the members of elmk_snicar_tables in order) and the snow-age tables.  The files
// of the elmk_run demos add "lat", "lon", "series/<field>" ([records][ncols]: hourly atm_*, twelve months of mlai .. mhbot) and
// "steps" (elmk_run_step rows); what else a demo reads, its head comment names.
#pragma once
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "elmk_interface.hpp"

namespace demo {

inline std::vector<char> read_all(const char* path)
{
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<char> b((size_t)n);
  if (std::fread(b.data(), 1, (size_t)n, f) != (size_t)n) throw std::runtime_error("short read");
  std::fclose(f);
  return b;
}

// the records of a state.bin by name; the pointers lead into `bytes`
struct Inputs {
  std::vector<char> bytes;
  int64_t ncols = 0;
  std::map<std::string, const char*> fields, params;
  std::map<std::string, int64_t> sizes;  // bytes of a record, fields and parameters alike

  explicit Inputs(const char* path) : bytes(read_all(path))
  {
    const char* p = bytes.data();
    const char* end = p + bytes.size();
    std::memcpy(&ncols, p, 8);
    p += 8;
    while (p < end) {
      char name[33] = {0};
      std::memcpy(name, p, 32);
      int32_t kind;
      int64_t nbytes;
      std::memcpy(&kind, p + 32, 4);
      std::memcpy(&nbytes, p + 36, 8);
      (kind == 0 ? fields : params)[name] = p + 44;
      sizes[name] = nbytes;
      p += 44 + nbytes;
    }
  }
  Inputs(const Inputs&) = delete;

  const double* D(const std::string& k) const { return reinterpret_cast<const double*>(params.at(k)); }
  const int32_t* I(const std::string& k) const { return reinterpret_cast<const int32_t*>(params.at(k)); }
  double dt() const { return D("scalars")[4]; }
};

// what every demo does before its own subject: land unit, scalars, PFT, soil colour, SNICAR and snow-age tables
inline void setup(elmk::ELMInterface& elm, const Inputs& in)
{
  elmk_snicar_tables t;
  std::memset(&t, 0, sizeof t);
  const double** slot = reinterpret_cast<const double**>(&t);  // the struct is 31 const double* members, in this order
  for (int i = 0; i < (int)(sizeof t / sizeof(double*)); i++) slot[i] = in.D("snicar/" + std::to_string(i));
  const int32_t* land = in.I("land");
  const double* sc = in.D("scalars");
  elm.setup(land[0], land[1], land[2], land[3], land[4], sc[0], (int)sc[1], sc[2], sc[3], in.D("pft_psn"), in.D("pft_alb"),
            in.D("z0mr"), in.D("displar"), in.D("albsat"), in.D("albdry"), &t, in.D("age_tau"), in.D("age_kappa"), in.D("age_drdt0"));
}

inline void upload_fields(elmk::ELMInterface& elm, const Inputs& in)
{
  for (const auto& kv : in.fields) elm.upload(kv.first.c_str(), kv.second);
}

// the series of an elmk_run: the forcing streams by record, the phenology by month
inline const char* const FORCING[] = {"atm_tbot", "atm_pbot", "atm_qbot", "atm_flds", "atm_fsds", "atm_prec", "atm_wind"};
inline const char* const PHENOLOGY[] = {"mlai", "msai", "mhtop", "mhbot"};

// every record of "series/<field>" to the device: nrec forcing records, twelve months; after reserve_run
inline void upload_series(elmk::ELMInterface& elm, const Inputs& in, int nrec)
{
  for (const char* f : FORCING) elm.series_upload(f, 0, nrec, in.D(std::string("series/") + f));
  for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, in.D(std::string("series/") + f));
}

// "steps" as rows; nsteps > 0: the file must hold exactly that many
inline std::vector<elmk_run_step> run_steps(const Inputs& in, int nsteps = 0)
{
  const int64_t bytes = in.sizes.at("steps"), row = (int64_t)sizeof(elmk_run_step);
  if (nsteps > 0 && bytes != nsteps * row) throw std::runtime_error("steps: expected " + std::to_string(nsteps) + " rows");
  if (bytes < row || bytes % row != 0) throw std::runtime_error("steps: not whole rows");
  std::vector<elmk_run_step> steps((size_t)(bytes / row));
  std::memcpy(steps.data(), in.params.at("steps"), (size_t)bytes);
  return steps;
}

// start-up of a context that runs the whole series: setup, the fields of the file (skipped when a restart image follows), geography,
// room for nrec records and nsteps steps, every record
inline void start(elmk::ELMInterface& elm, const Inputs& in, int nrec, int nsteps, bool fields = true)
{
  setup(elm, in);
  if (fields) upload_fields(elm, in);
  elm.set_column_geography(in.D("lat"), in.D("lon"));
  elm.reserve_run(nrec, nsteps);
  upload_series(elm, in, nrec);
}

}  // namespace demo
