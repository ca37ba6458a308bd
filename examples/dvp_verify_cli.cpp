// Host program over the C ABI only (include/dvpari.h): the designated verifier's half of the reference's lifecycle,
// `SRS::verify(secrets, public_inputs, proof)` (src/srs.rs:374-428), from files and the command line alone:
//
//   dvp_verify_cli <proof.bin> <tau> <delta> <epsilon> [<public input>...] [--srs-hash <hex>] [--circuit-hash <hex>] [--trace]
//
// --srs-hash / --circuit-hash (64 hex digits each): the binding the proof was made under (dvp_verify_set_binding; what
// dvp_prove_cli --bind-srs printed, and the host's circuit hash).  A hash that is not given is BLAKE3(""), the reference's transcript.
//
// --trace: after the verdict line, the verifier's stage values for this proof (dvp_verify_trace_batch), one `name = hex` line per
// field: alpha, i0, r0, u0, v0 and the coordinates p_x, p_y, k_x, ... sum_y as 64-digit numbers, the *_inf flags and the verdict as
// two digits.  The exit status does not change.
//
// proof.bin holds the 118 bytes of Proof::to_bytes (what dvp_prove_cli writes); the trapdoor values and the public inputs are
// canonical field elements in hex (an optional 0x prefix).  Exit status: 0 accepted, 2 rejected (the DVP_VERIFY_* reason bits
// are printed), 1 usage or I/O error, 3 no GPU.
//
// build:  g++ -O2 -std=c++17 -Iinclude examples/dvp_verify_cli.cpp -Ldv-pari_amd -ldvpari_hip -Wl,-rpath,$PWD/dv-pari_amd -o dvp_verify_cli
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dvpari.h"

// 4 x u64 little-endian limbs as one 64-digit number
static void print_limbs(const char* name, const char* suffix, const uint64_t v[4]) {
  printf("%s%s = %016llx%016llx%016llx%016llx\n", name, suffix, (unsigned long long)v[3], (unsigned long long)v[2], (unsigned long long)v[1],
         (unsigned long long)v[0]);
}

static void print_trace(const dvp_verify_trace& t) {
  const struct { const char* name; const uint64_t* v; } frs[] = {{"alpha", t.alpha}, {"i0", t.i0}, {"r0", t.r0}, {"u0", t.u0}, {"v0", t.v0}};
  for (const auto& f : frs) print_limbs(f.name, "", f.v);
  const struct { const char* name; const uint64_t* xy; uint8_t inf; } pts[] = {
      {"p", t.p_xy, t.p_inf}, {"k", t.k_xy, t.k_inf}, {"vk", t.vk_xy, t.vk_inf}, {"ug", t.ug_xy, t.ug_inf}, {"sum", t.sum_xy, t.sum_inf}};
  for (const auto& p : pts) {
    print_limbs(p.name, "_x", p.xy);
    print_limbs(p.name, "_y", p.xy + 4);
  }
  for (const auto& p : pts) printf("%s_inf = %02x\n", p.name, p.inf);
  printf("verdict = %02x\n", t.verdict);
}

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

// 64 hex digits (an optional 0x prefix) -> 32 bytes in the order written, as a digest is printed
static bool parse_hash(const char* s, uint8_t out[32]) {
  if (s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) s += 2;
  if (strlen(s) != 64) return false;
  for (int i = 0; i < 64; ++i) {
    const char c = s[i];
    int v;
    if (c >= '0' && c <= '9') v = c - '0';
    else if (c >= 'a' && c <= 'f') v = c - 'a' + 10;
    else if (c >= 'A' && c <= 'F') v = c - 'A' + 10;
    else return false;
    out[i / 2] = (uint8_t)((i & 1) ? (out[i / 2] | v) : (v << 4));
  }
  return true;
}

int main(int argc, char** argv) {
  bool have_hash[2] = {false, false}, trace = false;
  uint8_t hashes[2][32] = {{0}, {0}};
  std::vector<char*> pos;
  for (int i = 1; i < argc; ++i) {
    const int k = std::string(argv[i]) == "--srs-hash" ? 0 : std::string(argv[i]) == "--circuit-hash" ? 1 : -1;
    if (std::string(argv[i]) == "--trace") {
      trace = true;
    } else if (k < 0) {
      pos.push_back(argv[i]);
    } else if (i + 1 >= argc || !parse_hash(argv[i + 1], hashes[k])) {
      fprintf(stderr, "%s: expected 64 hex digits\n", argv[i]);
      return 1;
    } else {
      have_hash[k] = true;
      ++i;
    }
  }
  argc = (int)pos.size() + 1;
  for (size_t i = 0; i < pos.size(); ++i) argv[i + 1] = pos[i];
  if (argc < 5) {
    fprintf(stderr, "usage: %s <proof.bin> <tau> <delta> <epsilon> [<public input>...] [--srs-hash HEX] [--circuit-hash HEX] [--trace]   (hex, canonical)\n", argv[0]);
    return 1;
  }
  uint64_t td[3][4];
  for (int k = 0; k < 3; ++k)
    if (!parse_hex(argv[2 + k], td[k])) {
      fprintf(stderr, "not a hex value: %s\n", argv[2 + k]);
      return 1;
    }
  std::vector<uint64_t> pub(4 * (size_t)(argc - 5) + 4);
  for (int k = 5; k < argc; ++k)
    if (!parse_hex(argv[k], pub.data() + 4 * (size_t)(k - 5))) {
      fprintf(stderr, "not a hex value: %s\n", argv[k]);
      return 1;
    }
  uint8_t proof[119];
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "%s: cannot open\n", argv[1]);
    return 1;
  }
  const size_t got = fread(proof, 1, sizeof(proof), f);
  fclose(f);
  if (got != 118) {
    fprintf(stderr, "%s: %zu bytes, a proof has 118\n", argv[1], got);
    return 1;
  }
  if (dvp_device_count() <= 0) {
    fprintf(stderr, "no HIP device visible\n");
    return 3;
  }
  if (dvp_verify_set_binding(have_hash[0] ? hashes[0] : nullptr, have_hash[1] ? hashes[1] : nullptr) != DVP_OK) return 1;
  int accepted = 0;
  uint32_t reasons = 0;
  const int rc = dvp_verify(td[0], td[1], td[2], pub.data(), (uint32_t)(argc - 5), proof, &accepted, &reasons);
  if (rc != DVP_OK) {
    fprintf(stderr, "dvp_verify: %s (index %lld)\n", dvp_strerror(rc), (long long)dvp_last_error_index());
    return 1;
  }
  if (accepted) {
    printf("accepted\n");
  } else {
    std::string why;
    const struct { uint32_t bit; const char* name; } names[] = {
        {DVP_VERIFY_BAD_COMMIT_P, "bad_commit_p"}, {DVP_VERIFY_BAD_KZG_K, "bad_kzg_k"}, {DVP_VERIFY_BAD_A0, "bad_a0"},
        {DVP_VERIFY_BAD_B0, "bad_b0"}, {DVP_VERIFY_BAD_PUBLIC, "bad_public"}, {DVP_VERIFY_EQUATION, "equation"}};
    for (const auto& n : names)
      if (reasons & n.bit) why += std::string(why.empty() ? "" : ",") + n.name;
    printf("rejected 0x%02x %s\n", reasons, why.c_str());
  }
  if (trace) {
    dvp_verify_trace t;
    const int rt = dvp_verify_trace_batch(td[0], td[1], td[2], pub.data(), (uint32_t)(argc - 5), proof, 1, &t);
    if (rt != DVP_OK) {
      fprintf(stderr, "dvp_verify_trace_batch: %s\n", dvp_strerror(rt));
      return 1;
    }
    print_trace(t);
  }
  return accepted ? 0 : 2;
}
