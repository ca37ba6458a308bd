// Host program over the C ABI only (include/dvpari.h): what a compiled-language maintainer -- the reference is Rust -- links
// against.  It mirrors the reference's `Proof::prove(cache_dir, public_inputs, private_inputs)` call
// (src/proving.rs:426) from files alone:
//
//   dvp_prove_cli <cache_dir> <n_public> [<proof_out>] [--devices 0,1,2,3] [--table-budget <bytes>] [--bind-srs] [--bind-circuit | --circuit-hash <hex>]
//                 [--host-witness] [--repeat N --threads T] [--trace] [--also <srs_dir>]...
//   dvp_prove_cli <cache_dir> <n_public> --check-witness [--max-rows N]
//
// --check-witness: explain the witness instead of proving (dvp_check_witness_cache_dir_witness_file; needs the dump and the witness
// file, no SRS file).  Prints the counts, then up to N failing rows and N suspect wires (default 16); exit status 0 when the witness
// satisfies every row with entries below p, else 2.
//
// The witness goes from the file to the proof in one call, dvp_prove_cache_dir_witness_file: the library maps
// <cache_dir>/witness_to_dvsnark and reduces its elements mod p on the GPU.  --host-witness keeps the two-step path a host used before
// that entry existed: dvp_file_witness_read (reduction on one host thread) + dvp_prover_open_cache_dir + dvp_prove.  Same bytes.
// --repeat N --threads T: N more proofs through dvp_prove_cache_dir with the witness as limbs in host memory, whichever way the first
// proof went; the witness is read and reduced on the host only for this leg or under --host-witness.
//
// --trace: after the proof line, the stages of that proof (dvp_prover_trace_last with DVP_TRACE_ALL) as `name = hex` lines -- the header
// words, alpha, z_alpha, a0, b0, i0, r0, the seven points (x, y, infinity flag, 30-byte encoding) and the sixteen vector digests under
// the names src/proving.rs gives the vectors: what a host compares field by field when its reference prover's bytes differ
// ("When the bytes differ").  Single device only; it costs more than the proof.
//
// --also <srs_dir> (repeatable): one witness, one proof per verifier.  Each <srs_dir> holds another verifier's SRS for the same circuit
// (its g_m, g_q, g_k_0..2; an R1CS dump there must be the same circuit): dvp_cache_dir_add_srs_dir puts it into a slot of cache_dir's
// prover and dvp_prove_cache_dir_multi_witness_file proves for cache_dir's own SRS and then for each --also, in order, with the
// first phase of the proof, which does not depend on the SRS, computed once.  Prints one line per verifier, `<directory>
// <118 bytes in hex>`; exit status 0 only if every proof was made.  --table-budget, the bindings, <proof_out> and --trace keep acting
// on the first proof, cache_dir's own (under --trace that proof is made last, so that the trace is its trace).  Excludes
// --host-witness, --repeat and --devices.
//
// --bind-srs: bind the proof's challenge to the SRS (dvp_prover_srs_hash + dvp_prover_set_transcript_binding); the SRS hash used goes
// to stderr -- the verifier needs it (dvp_verify_cli --srs-hash).  --circuit-hash <64 hex digits>: the circuit half of the binding
// (whatever the host defines it to be).  --bind-circuit: the circuit half is dvp_prover_circuit_hash of the prover, the hash of the
// stream Transcript::circuit_info_hash would build (coeff_ids per row and the coefficient table, Vandermonde terms included); it goes to
// stderr as well (dvp_verify_cli --circuit-hash; a verifier computes the same value with dvp_circuit_hash_cache_dir).  It excludes
// --circuit-hash.  Without any of them the transcript is the reference's, which binds neither.
//
// --table-budget <bytes>: the most HBM per device the prover's fixed-base tables may hold (dvp_prover_set_table_budget; 0 = no
// tables).  What does not fit runs through the one-shot MSM; the proof bytes do not depend on it.  The coverage goes to stderr.
//
// --devices d0,d1,..: in-library multi-GPU (dvp_set_devices): the two MSMs of the proof are sharded over the listed
// devices, one host thread each; d0 is the home device.  An id may repeat.  The proof bytes do not depend on the list.
//
// reads <cache_dir>/witness_to_dvsnark (u32-BE count || 32-byte BE elements = [1, public.., private..],
// src/gnark_r1cs.rs:188-210), lets the library open the R1CS dump and the SRS point files of the same directory, proves on
// the GPU and prints the 118 proof bytes in hex (optionally also writes them to <proof_out>).
//
// build:  g++ -O2 -std=c++17 -Iinclude examples/dvp_prove_cli.cpp -Ldv-pari_amd -ldvpari_hip -Wl,-rpath,$PWD/dv-pari_amd -o dvp_prove_cli
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "dvpari.h"

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

// the record as `name = hex` lines: header words, scalars and coordinates as big-endian numbers, encodings and digests byte by byte
static void print_trace(const dvp_prove_trace& t) {
  const struct { const char* name; uint32_t v; } hdr[] = {{"log2_m", t.log2_m}, {"n_wires", t.n_wires}, {"n_public", t.n_public},
                                                            {"codec_rule", t.codec_rule}, {"parts", t.parts}, {"mismatch", t.mismatch}};
  for (const auto& h : hdr) printf("%s = %08x\n", h.name, h.v);
  auto num = [](const char* name, const char* suffix, const uint64_t v[4]) {
    printf("%s%s = %016llx%016llx%016llx%016llx\n", name, suffix, (unsigned long long)v[3], (unsigned long long)v[2], (unsigned long long)v[1],
           (unsigned long long)v[0]);
  };
  auto bytes = [](const char* name, const char* suffix, const uint8_t* b, int n) {
    printf("%s%s = ", name, suffix);
    for (int i = 0; i < n; ++i) printf("%02x", b[i]);
    printf("\n");
  };
  const struct { const char* name; const uint64_t* v; } sc[] = {{"alpha", t.alpha}, {"z_alpha", t.z_alpha}, {"a0", t.a0},
                                                                 {"b0", t.b0},       {"i0", t.i0},           {"r0", t.r0}};
  for (const auto& s : sc) num(s.name, "", s.v);
  const struct { const char* name; const dvp_trace_point* p; } pt[] = {{"msm_gm", &t.msm_gm}, {"msm_q", &t.msm_q}, {"commit_p", &t.commit_p},
                                                                        {"kzg_a", &t.kzg_a},   {"kzg_b", &t.kzg_b}, {"kzg_r", &t.kzg_r},
                                                                        {"kzg_k", &t.kzg_k}};
  for (const auto& q : pt) {
    num(q.name, "_x", q.p->xy);
    num(q.name, "_y", q.p->xy + 4);
    printf("%s_inf = %02x\n", q.name, q.p->inf);
    bytes(q.name, "_enc", q.p->enc, 30);
  }
  const struct { const char* name; const uint8_t* d; } dg[] = {
      {"assignment", t.assignment}, {"evals.a", t.evals_a},         {"evals.b", t.evals_b},         {"evals.c", t.evals_c},
      {"evals.i", t.evals_i},       {"evals2.a", t.evals2_a},       {"evals2.b", t.evals2_b},       {"evals2.c", t.evals2_c},
      {"evals2.i", t.evals2_i},     {"r_vals2", t.r_vals2},         {"q_vals2", t.q_vals2},         {"denom_invs", t.denom_invs},
      {"denom_invs2", t.denom_invs2}, {"k_scalar_a", t.k_scalar_a}, {"k_scalar_b", t.k_scalar_b},   {"k_scalar_r", t.k_scalar_r}};
  for (const auto& d : dg) bytes(d.name, "", d.d, 32);
}

int main(int argc, char** argv) {
  std::vector<int> devices;
  bool bind_srs = false, bind_circuit = false, have_circuit = false, host_witness = false;
  uint8_t srs_hash[32] = {0}, circuit_hash[32] = {0};
  int repeat = 0, threads = 1;  // --repeat N --threads T: N more proofs through dvp_prove_cache_dir from T host threads
  bool check_witness = false;   // --check-witness [--max-rows N]: explain the witness instead of proving
  size_t max_rows = 16;
  bool trace = false;           // --trace: print the stages of the proof behind the proof line
  dvp_prove_trace tr;
  std::vector<char*> pos;
  std::vector<std::string> also;  // --also <srs_dir>: further verifiers' SRS directories
  bool have_budget = false;
  uint64_t budget = UINT64_MAX;
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--table-budget" && i + 1 < argc) {
      char* end = nullptr;
      const unsigned long long v = strtoull(argv[++i], &end, 10);
      if (end == argv[i] || *end != 0 || argv[i][0] == '-') {
        fprintf(stderr, "--table-budget: expected a number of bytes, got '%s'\n", argv[i]);
        return 2;
      }
      budget = (uint64_t)v;
      have_budget = true;
    } else if (std::string(argv[i]) == "--also" && i + 1 < argc) {
      also.push_back(argv[++i]);
    } else if (std::string(argv[i]) == "--bind-srs") {
      bind_srs = true;
    } else if (std::string(argv[i]) == "--bind-circuit") {
      bind_circuit = true;
    } else if (std::string(argv[i]) == "--host-witness") {
      host_witness = true;
    } else if (std::string(argv[i]) == "--trace") {
      trace = true;
    } else if (std::string(argv[i]) == "--check-witness") {
      check_witness = true;
    } else if (std::string(argv[i]) == "--max-rows" && i + 1 < argc) {
      char* end = nullptr;
      const long v = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end != 0 || v < 0 || v > 1000000) {
        fprintf(stderr, "--max-rows: expected a count, got '%s'\n", argv[i]);
        return 2;
      }
      max_rows = (size_t)v;
    } else if (std::string(argv[i]) == "--circuit-hash" && i + 1 < argc) {
      if (!parse_hash(argv[++i], circuit_hash)) {
        fprintf(stderr, "--circuit-hash: expected 64 hex digits, got '%s'\n", argv[i]);
        return 2;
      }
      have_circuit = true;
    } else if (std::string(argv[i]) == "--devices" && i + 1 < argc) {
      for (char* tok = argv[++i]; *tok;) {
        char* end = tok;
        const long id = strtol(tok, &end, 10);
        if (end == tok || (*end != ',' && *end != 0) || id < 0 || id > 1023) {  // not a number / stray character: do not spin on it
          fprintf(stderr, "--devices: expected a comma-separated list of device ids, got '%s'\n", argv[i]);
          return 2;
        }
        devices.push_back((int)id);
        tok = *end == ',' ? end + 1 : end;
      }
    } else if ((std::string(argv[i]) == "--repeat" || std::string(argv[i]) == "--threads") && i + 1 < argc) {
      const bool rep = std::string(argv[i]) == "--repeat";
      char* end = nullptr;
      const long v = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end != 0 || v < 1 || v > 1000000) {
        fprintf(stderr, "%s: expected a positive number, got '%s'\n", rep ? "--repeat" : "--threads", argv[i]);
        return 2;
      }
      (rep ? repeat : threads) = (int)v;
    } else {
      pos.push_back(argv[i]);
    }
  }
  if (bind_circuit && have_circuit) fprintf(stderr, "--bind-circuit and --circuit-hash exclude each other\n");
  const bool also_clash = !also.empty() && (host_witness || repeat > 0 || !devices.empty());
  if (also_clash) fprintf(stderr, "--also excludes --host-witness, --repeat and --devices\n");
  if (pos.size() < 2 || (bind_circuit && have_circuit) || also_clash) {
    fprintf(stderr, "usage: %s <cache_dir> <n_public> [<proof_out>] [--devices 0,1,..] [--table-budget BYTES] [--bind-srs] [--bind-circuit | --circuit-hash HEX] [--host-witness] [--repeat N --threads T] [--trace] [--also SRS_DIR]... | --check-witness [--max-rows N]\n", argv[0]);
    return 2;
  }
  argc = (int)pos.size() + 1;
  for (size_t i = 0; i < pos.size(); ++i) argv[i + 1] = pos[i];
  const std::string dir = argv[1];
  const uint32_t n_public = (uint32_t)strtoul(argv[2], nullptr, 10);
  if (dvp_device_count() <= 0) {
    fprintf(stderr, "no HIP device visible (the library has no CPU path)\n");
    return 3;
  }
  if (!devices.empty()) {
    int rcd = dvp_set_device(devices[0]);
    if (rcd == DVP_OK) rcd = dvp_set_devices(devices.data(), (int)devices.size());
    if (rcd != DVP_OK) {
      fprintf(stderr, "--devices: %s\n", dvp_strerror(rcd));
      return 1;
    }
  }
  if (check_witness) {
    // Why would this witness be refused?  dvp_check_witness_cache_dir_witness_file reads the dump and the witness file, no SRS file,
    // and proves nothing: one line of counts, one line per listed failing row (a*b != c + i) and per suspect wire (a wire whose terms
    // all lie in failing rows).  Exit status 0 when every row holds and every entry is below p, else 2.
    std::vector<dvp_unsat_row> rows(max_rows ? max_rows : 1);
    std::vector<dvp_suspect_wire> wires(max_rows ? max_rows : 1);
    dvp_witness_report rep;
    const int rcw = dvp_check_witness_cache_dir_witness_file(dir.c_str(), n_public, nullptr, max_rows ? rows.data() : nullptr, max_rows,
                                                             max_rows ? wires.data() : nullptr, max_rows, &rep);
    if (rcw != DVP_OK) {
      fprintf(stderr, "check %s: %s (index %lld)\n", dir.c_str(), dvp_strerror(rcw), (long long)dvp_last_error_index());
      return 1;
    }
    printf("witness: n_unsat=%llu first_unsat=%lld n_noncanonical=%llu first_noncanonical=%lld n_suspect_wires=%llu constant_wire_is_one=%u\n",
           (unsigned long long)rep.n_unsat, (long long)rep.first_unsat, (unsigned long long)rep.n_noncanonical,
           (long long)rep.first_noncanonical, (unsigned long long)rep.n_suspect_wires, rep.constant_wire_is_one);
    auto hex = [](const uint64_t v[4]) { printf("0x%016llx%016llx%016llx%016llx", (unsigned long long)v[3], (unsigned long long)v[2], (unsigned long long)v[1], (unsigned long long)v[0]); };
    for (uint32_t k = 0; k < rep.n_rows_listed; ++k) {
      printf("row %llu a=", (unsigned long long)rows[k].row);
      hex(rows[k].a);
      printf(" b=");
      hex(rows[k].b);
      printf(" c=");
      hex(rows[k].c);
      printf(" i=");
      hex(rows[k].i);
      printf("\n");
    }
    for (uint32_t k = 0; k < rep.n_wires_listed; ++k) printf("wire %u n_terms=%u\n", wires[k].wire, wires[k].n_terms);
    dvp_cache_dir_release(nullptr);
    return rep.n_unsat == 0 && rep.n_noncanonical == 0 && rep.constant_wire_is_one ? 0 : 2;
  }
  const std::string wpath = dir + "/witness_to_dvsnark";
  uint8_t proof[118];
  std::vector<uint64_t> w;  // the witness as canonical limbs, read and reduced on the host: --host-witness and --repeat only
  size_t n = 0, n_wires = 0;
  int rc = DVP_OK;
  if (host_witness || repeat > 0) {
    rc = dvp_file_witness_read(wpath.c_str(), nullptr, 0, &n);
    if (rc != DVP_OK) {
      fprintf(stderr, "%s: %s\n", wpath.c_str(), dvp_strerror(rc));
      return 1;
    }
    w.resize(4 * n);
    rc = dvp_file_witness_read(wpath.c_str(), w.data(), n, &n);
    if (rc != DVP_OK || n < 1 + (size_t)n_public) {
      fprintf(stderr, "witness: %s (n = %zu)\n", dvp_strerror(rc), n);
      return 1;
    }
    if (w[0] != 1 || w[1] || w[2] || w[3]) {
      fprintf(stderr, "witness[0] must be the constant 1 (src/proving.rs:449-452)\n");
      return 1;
    }
  }
  if (!host_witness) {
    // load_witness_from_file + Proof::prove as ONE call: the library maps the file and reduces its elements mod p on the GPU.  The
    // prover is the one the library keeps for this directory, so the budget and the binding go to that one.
    dvp_prover* cp = nullptr;
    if (have_budget || bind_srs || bind_circuit || trace) {
      rc = dvp_cache_dir_prover(dir.c_str(), n_public, &cp);
      if (rc != DVP_OK) {
        fprintf(stderr, "open %s: %s (index %lld)\n", dir.c_str(), dvp_strerror(rc), (long long)dvp_last_error_index());
        return 1;
      }
    }
    if (have_budget) {
      rc = dvp_prover_set_table_budget(cp, budget);
      if (rc != DVP_OK) {
        fprintf(stderr, "--table-budget: %s\n", dvp_strerror(rc));
        return 1;
      }
    }
    if (bind_srs || have_circuit || bind_circuit) {
      rc = bind_srs ? dvp_prover_srs_hash(cp, srs_hash) : DVP_OK;
      if (rc == DVP_OK && bind_circuit) {
        rc = dvp_prover_circuit_hash(cp, circuit_hash);
        have_circuit = rc == DVP_OK;
      }
      if (rc == DVP_OK) rc = dvp_cache_dir_set_binding(dir.c_str(), n_public, bind_srs ? srs_hash : nullptr, have_circuit ? circuit_hash : nullptr, 0);
      if (rc != DVP_OK) {
        fprintf(stderr, "--bind-srs / --bind-circuit / --circuit-hash: %s\n", dvp_strerror(rc));
        return 1;
      }
      if (bind_srs) {
        fprintf(stderr, "srs hash: ");
        for (int i = 0; i < 32; ++i) fprintf(stderr, "%02x", srs_hash[i]);
        fprintf(stderr, "\n");
      }
      if (bind_circuit) {
        fprintf(stderr, "circuit hash: ");
        for (int i = 0; i < 32; ++i) fprintf(stderr, "%02x", circuit_hash[i]);
        fprintf(stderr, "\n");
      }
    }
    std::vector<uint8_t> more(118 * also.size());  // the proofs for the --also directories, in their order
    if (also.empty()) {
      rc = dvp_prove_cache_dir_witness_file(dir.c_str(), n_public, nullptr, proof, nullptr);
    } else {
      // slot 0 is cache_dir's own SRS; under --trace it goes last, so that the prover's last proof is the one the trace is asked for
      std::vector<uint32_t> slots(1 + also.size(), 0);
      const size_t first = trace ? also.size() : 0, others = trace ? 0 : 1;
      for (size_t k = 0; k < also.size(); ++k) {
        rc = dvp_cache_dir_add_srs_dir(dir.c_str(), n_public, also[k].c_str(), &slots[others + k]);
        if (rc != DVP_OK) {
          fprintf(stderr, "--also %s: %s\n", also[k].c_str(), dvp_strerror(rc));
          return 1;
        }
      }
      std::vector<uint8_t> all(118 * slots.size());
      std::vector<int32_t> status(slots.size(), DVP_OK);
      rc = dvp_prove_cache_dir_multi_witness_file(dir.c_str(), n_public, slots.data(), (uint32_t)slots.size(), nullptr, all.data(), status.data(),
                                                  nullptr);
      for (size_t k = 0; rc == DVP_OK && k < slots.size(); ++k)
        if (status[k] != DVP_OK) {
          fprintf(stderr, "prove for %s: %s\n", k == first ? dir.c_str() : also[k - others].c_str(), dvp_strerror(status[k]));
          rc = status[k];
        }
      if (rc == DVP_OK) {
        memcpy(proof, all.data() + 118 * first, 118);
        memcpy(more.data(), all.data() + 118 * others, more.size());
      }
    }
    if (rc != DVP_OK) {
      fprintf(stderr, "prove from %s: %s (index %lld)\n", wpath.c_str(), dvp_strerror(rc), (long long)dvp_last_error_index());
      return 1;
    }
    if (!also.empty()) {
      printf("%s ", dir.c_str());
      for (int i = 0; i < 118; ++i) printf("%02x", proof[i]);
      printf("\n");
      for (size_t k = 0; k < also.size(); ++k) {
        printf("%s ", also[k].c_str());
        for (int i = 0; i < 118; ++i) printf("%02x", more[118 * k + i]);
        printf("\n");
      }
    }
    if (trace && (rc = dvp_prover_trace_last(cp, DVP_TRACE_ALL, &tr, nullptr)) != DVP_OK) {
      fprintf(stderr, "--trace: %s\n", dvp_strerror(rc));
      return 1;
    }
    if (have_budget)
      for (int which = 1; which >= 0; --which) {
        size_t covered = 0, total = 0;
        int reason = 0;
        if (dvp_prover_msm_coverage(cp, which, &covered, &total, &reason) == DVP_OK)
          fprintf(stderr, "MSM %d: %zu of %zu bases from tables (%llu bytes)%s\n", which, covered, total,
                  (unsigned long long)dvp_prover_msm_table_bytes(cp, which, nullptr),
                  reason == 1 ? ", limited by the budget" : reason == 2 ? ", table refused by the runtime" : "");
      }
    if (repeat > 0) {  // the repeat leg hands limbs to dvp_prove_cache_dir: it needs the commitment key's length, as below
      if (!cp) rc = dvp_cache_dir_prover(dir.c_str(), n_public, &cp);
      if (rc != DVP_OK) {
        fprintf(stderr, "open %s: %s\n", dir.c_str(), dvp_strerror(rc));
        return 1;
      }
      n_wires = dvp_prover_msm_size(cp, 0) - dvp_prover_msm_size(cp, 1) / 4;
      if (n_wires < 1 + (size_t)n_public || n_wires > n) {
        fprintf(stderr, "witness has %zu entries, the commitment key wants %zu\n", n, n_wires);
        return 1;
      }
    } else {
      dvp_cache_dir_release(nullptr);
    }
  } else {
    // The dump knows wires only up to the highest one used; the library takes the witness length from |g_m|, so hand over
    // exactly that many private inputs (a longer witness file is truncated by the reference's zip as well).
    dvp_prover* p = nullptr;
    rc = dvp_prover_open_cache_dir(dir.c_str(), n_public, &p);
    if (rc != DVP_OK) {
      fprintf(stderr, "open %s: %s (index %lld)\n", dir.c_str(), dvp_strerror(rc), (long long)dvp_last_error_index());
      return 1;
    }
    // |[w | q2]| = n_wires + m and |[k_a | k_b | k_r]| = 4m
    n_wires = dvp_prover_msm_size(p, 0) - dvp_prover_msm_size(p, 1) / 4;
    if (n_wires < 1 + (size_t)n_public || n_wires > n) {
      fprintf(stderr, "witness has %zu entries, the commitment key wants %zu\n", n, n_wires);
      dvp_prover_destroy(p);
      return 1;
    }
    if (have_budget) {
      rc = dvp_prover_set_table_budget(p, budget);
      if (rc != DVP_OK) {
        fprintf(stderr, "--table-budget: %s\n", dvp_strerror(rc));
        dvp_prover_destroy(p);
        return 1;
      }
    }
    if (bind_srs || have_circuit || bind_circuit) {
      rc = bind_srs ? dvp_prover_srs_hash(p, srs_hash) : DVP_OK;
      if (rc == DVP_OK && bind_circuit) {
        rc = dvp_prover_circuit_hash(p, circuit_hash);
        have_circuit = rc == DVP_OK;
      }
      if (rc == DVP_OK) rc = dvp_prover_set_transcript_binding(p, bind_srs ? srs_hash : nullptr, have_circuit ? circuit_hash : nullptr);
      if (rc != DVP_OK) {
        fprintf(stderr, "--bind-srs / --bind-circuit / --circuit-hash: %s\n", dvp_strerror(rc));
        dvp_prover_destroy(p);
        return 1;
      }
      if (bind_srs) {
        fprintf(stderr, "srs hash: ");
        for (int i = 0; i < 32; ++i) fprintf(stderr, "%02x", srs_hash[i]);
        fprintf(stderr, "\n");
      }
      if (bind_circuit) {
        fprintf(stderr, "circuit hash: ");
        for (int i = 0; i < 32; ++i) fprintf(stderr, "%02x", circuit_hash[i]);
        fprintf(stderr, "\n");
      }
    }
    rc = dvp_prove(p, w.data() + 4, n_public, w.data() + 4 * (1 + (size_t)n_public), (uint32_t)(n_wires - 1 - n_public), proof);
    if (have_budget && rc == DVP_OK)
      for (int which = 1; which >= 0; --which) {
        size_t covered = 0, total = 0;
        int reason = 0;
        if (dvp_prover_msm_coverage(p, which, &covered, &total, &reason) == DVP_OK)
          fprintf(stderr, "MSM %d: %zu of %zu bases from tables (%llu bytes)%s\n", which, covered, total,
                  (unsigned long long)dvp_prover_msm_table_bytes(p, which, nullptr),
                  reason == 1 ? ", limited by the budget" : reason == 2 ? ", table refused by the runtime" : "");
      }
    if (trace && rc == DVP_OK && (rc = dvp_prover_trace_last(p, DVP_TRACE_ALL, &tr, nullptr)) != DVP_OK) {
      fprintf(stderr, "--trace: %s\n", dvp_strerror(rc));
      dvp_prover_destroy(p);
      return 1;
    }
    dvp_prover_destroy(p);
    if (rc != DVP_OK) {
      fprintf(stderr, "prove: %s (index %lld)\n", dvp_strerror(rc), (long long)dvp_last_error_index());
      return 1;
    }
  }
  if (also.empty()) {
    for (int i = 0; i < 118; ++i) printf("%02x", proof[i]);
    printf("\n");
  }
  if (trace) print_trace(tr);
  if (repeat > 0) {
    // Throughput through the reference's own signature (Proof::prove(cache_dir, public, private) = dvp_prove_cache_dir): `threads`
    // host threads share `repeat` proofs; with two or more, the library keeps two proofs in flight on the GPU.  Every proof must
    // equal the first one.
    const uint64_t* pub = w.data() + 4;
    const uint64_t* prv = w.data() + 4 * (1 + (size_t)n_public);
    const uint32_t n_prv = (uint32_t)(n_wires - 1 - n_public);
    uint8_t warm[118];
    if (have_budget) {  // the prover dvp_prove_cache_dir keeps for this directory (a second one, DVP_CACHE_REPLICAS=2, starts from DVP_TABLE_BUDGET_BYTES)
      dvp_prover* cp = nullptr;
      rc = dvp_cache_dir_prover(dir.c_str(), n_public, &cp);
      if (rc == DVP_OK) rc = dvp_prover_set_table_budget(cp, budget);
      if (rc != DVP_OK) {
        fprintf(stderr, "--table-budget: %s\n", dvp_strerror(rc));
        return 1;
      }
    }
    if (bind_srs || have_circuit) {  // the same binding for the prover(s) dvp_prove_cache_dir keeps
      rc = dvp_cache_dir_set_binding(dir.c_str(), n_public, bind_srs ? srs_hash : nullptr, have_circuit ? circuit_hash : nullptr, 0);
      if (rc != DVP_OK) {
        fprintf(stderr, "dvp_cache_dir_set_binding: %s\n", dvp_strerror(rc));
        return 1;
      }
    }
    for (int t = 0; t < 2; ++t) {  // opens the cache_dir entry (and, below, its second prover) outside the timed part
      rc = dvp_prove_cache_dir(dir.c_str(), pub, n_public, prv, n_prv, warm);
      if (rc != DVP_OK || memcmp(warm, proof, 118)) {
        fprintf(stderr, "dvp_prove_cache_dir: %s\n", rc ? dvp_strerror(rc) : "bytes differ from dvp_prove");
        return 1;
      }
    }
    std::atomic<int> next(0), bad(0);
    auto worker = [&](int limit) {
      uint8_t out[118];
      while (next.fetch_add(1) < limit) {
        const int r = dvp_prove_cache_dir(dir.c_str(), pub, n_public, prv, n_prv, out);
        if (r != DVP_OK || memcmp(out, proof, 118)) bad.fetch_add(1);
      }
    };
    auto run = [&](int limit) {
      next = 0;
      std::vector<std::thread> th;
      for (int t = 0; t < threads; ++t) th.emplace_back(worker, limit);
      for (auto& t : th) t.join();
    };
    run(2 * threads);  // concurrent warm-up: the second prover of the entry is opened when two calls first overlap
    const auto t0 = std::chrono::steady_clock::now();
    run(repeat);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (bad.load()) {
      fprintf(stderr, "%d of the repeated proofs failed or differ\n", bad.load());
      return 1;
    }
    fprintf(stderr, "%d proofs from %d host thread(s): %.2f ms per proof (witness in host memory, dvp_prove_cache_dir)\n", repeat, threads, ms / repeat);
    dvp_cache_dir_release(nullptr);
  }
  if (argc > 3) {
    FILE* f = fopen(argv[3], "wb");
    if (!f || fwrite(proof, 1, 118, f) != 118) {
      fprintf(stderr, "cannot write %s\n", argv[3]);
      return 1;
    }
    fclose(f);
  }
  return 0;
}
