// Host program over the C ABI only (include/dvpari.h): the designated verifier's setup half of the reference's lifecycle,
// `SRS::verifier_runs_setup(trapdoor, cache_dir, num_public_inputs, ..)` (src/srs.rs:177-361), and the audit of its result:
//
//   dvp_setup_cli <cache_dir> <n_public> <tau> <delta> <epsilon> [--precomputes] [--check [--exact]]
//
// Without --check it reads <cache_dir>/r1cs_to_dvsnark and writes g_m, g_q, g_k_0, g_k_1, g_k_2 there (dvp_setup_cache_dir), with
// --precomputes also the six domain files.  With --check nothing is written: the five vectors found in <cache_dir> are checked
// against the trapdoor (dvp_srs_check_cache_dir: one combined MSM per vector; --exact compares every point instead) and one line per
// vector is printed.  The trapdoor values are canonical field elements in hex (an optional 0x prefix).
// Exit status: 0 the setup ran / the directory holds this trapdoor's SRS, 2 the audit found a bad vector, 1 usage or a failed call,
// 3 no GPU.
//
// build:  g++ -O2 -std=c++17 -Iinclude examples/dvp_setup_cli.cpp -Ldv-pari_amd -ldvpari_hip -Wl,-rpath,$PWD/dv-pari_amd -o dvp_setup_cli
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dvpari.h"

// hex -> 4 x u64 little-endian limbs; false for anything that is not 1..64 hex digits
static bool parse_hex(const char* s, uint64_t out[4]) {
  if (s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) s += 2;
  const size_t len = strlen(s);
  if (len == 0 || len > 64) return false;
  memset(out, 0, 32);
  for (size_t i = 0; i < len; ++i) {
    const char c = s[len - 1 - i];
    uint64_t v;
    if (c >= '0' && c <= '9') v = (uint64_t)(c - '0');
    else if (c >= 'a' && c <= 'f') v = (uint64_t)(c - 'a' + 10);
    else if (c >= 'A' && c <= 'F') v = (uint64_t)(c - 'A' + 10);
    else return false;
    out[i / 16] |= v << (4 * (i % 16));
  }
  return true;
}

int main(int argc, char** argv) {
  bool precomputes = false, audit = false, exact = false;
  std::vector<char*> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string a(argv[i]);
    if (a == "--precomputes") precomputes = true;
    else if (a == "--check") audit = true;
    else if (a == "--exact") exact = true;
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 5 || (exact && !audit) || (audit && precomputes)) {
    fprintf(stderr, "usage: %s <cache_dir> <n_public> <tau> <delta> <epsilon> [--precomputes] [--check [--exact]]   (hex, canonical)\n", argv[0]);
    return 1;
  }
  char* end = nullptr;
  const unsigned long n_public = strtoul(pos[1], &end, 10);
  if (!*pos[1] || *end || n_public > 0xfffffffful) {
    fprintf(stderr, "not a count: %s\n", pos[1]);
    return 1;
  }
  uint64_t td[3][4];
  for (int k = 0; k < 3; ++k)
    if (!parse_hex(pos[2 + k], td[k])) {
      fprintf(stderr, "not a hex value: %s\n", pos[2 + k]);
      return 1;
    }
  if (dvp_device_count() <= 0) {
    fprintf(stderr, "no HIP device visible\n");
    return 3;
  }
  if (!audit) {
    const int rc = dvp_setup_cache_dir(td[0], td[1], td[2], pos[0], (uint32_t)n_public, precomputes ? 1 : 0);
    if (rc != DVP_OK) {
      fprintf(stderr, "dvp_setup_cache_dir: %s (index %lld)\n", dvp_strerror(rc), (long long)dvp_last_error_index());
      return 1;
    }
    printf("setup written to %s\n", pos[0]);
    return 0;
  }
  dvp_srs_check_report rep;
  const int rc = dvp_srs_check_cache_dir(td[0], td[1], td[2], pos[0], (uint32_t)n_public, nullptr, exact ? DVP_SRS_CHECK_EXACT : 0u, &rep);
  if (rc != DVP_OK) {
    fprintf(stderr, "dvp_srs_check_cache_dir: %s (index %lld)\n", dvp_strerror(rc), (long long)dvp_last_error_index());
    return 1;
  }
  static const char* const names[5] = {"g_m", "g_q", "g_k_0", "g_k_1", "g_k_2"};
  static const char* const status[6] = {"ok", "missing", "length", "decode", "bad_point", "wrong"};
  static const char* const path[4] = {"-", "combined", "located", "exact"};
  for (int v = 0; v < 5; ++v) {
    printf("%-5s %-9s %-8s entries %llu", names[v], status[rep.status[v] < 6 ? rep.status[v] : 5], path[rep.path[v] < 4 ? rep.path[v] : 0],
           (unsigned long long)rep.count[v]);
    if (rep.first_bad[v] >= 0) printf(" first_bad %lld", (long long)rep.first_bad[v]);
    printf("\n");
  }
  if (!rep.verdict) {
    printf("accepted\n");
    return 0;
  }
  printf("rejected 0x%02x\n", rep.bad_vectors);
  return 2;
}
