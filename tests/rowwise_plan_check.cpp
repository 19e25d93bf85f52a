// Host check of picotron_amd/csrc/rowwise_plan.h (no HIP, CPU only; built and run by tests/test_rowwise_plan.py and
// tests/test_rowwise_host.py).
//
// Without arguments: the FastDiv sweep. fdiv(n, make_fastdiv(d)) == n / d for every d in 1..4096, every power of two
// +-1 up to 2^30 and a few thousand random d, at n in {0, 1, d-1, d, d+1, k d - 1, k d for sampled k, 2^31-2, 2^31-1}
// plus random n < 2^31. Prints "ok: <checks>" or the first mismatch (exit 1).
//
// With arguments (or "-" to read them from stdin, one per line): for each case, which instantiation and how many
// loop trips it reaches, one line "case key=value ..." each:
//   rms_fwd:ROWS:COLS            rms_bwd:ROWS:COLS:RES        rms_chain:ROWS:COLS:PREV_COLS
//   ce:THREADS:VOCAB             swiglu:ROWS:COLS:IS:OS:MISALIGN_BYTES
//   rope:B:S:H:D                 scale:N                      emb:DIM
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../picotron_amd/csrc/rowwise_plan.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

long long checks = 0;

bool check_n(unsigned d, const rw::FastDiv& f, uint64_t n) {
  if (n >= (1ull << 31)) return true;  // outside the claimed domain
  ++checks;
  const unsigned got = rw::fdiv((unsigned)n, f);
  if (got == (unsigned)n / d) return true;
  std::printf("FAIL: fdiv(%llu, %u) = %u, expected %u (m %u, l %u)\n", (unsigned long long)n, d, got, (unsigned)n / d,
              f.m, f.l);
  return false;
}

bool check_d(unsigned d) {
  const rw::FastDiv f = rw::make_fastdiv(d);
  const uint64_t top = (1ull << 31) - 1;
  const uint64_t fixed[] = {0, 1, (uint64_t)d - 1, d, (uint64_t)d + 1, top - 1, top};
  for (uint64_t n : fixed)
    if (!check_n(d, f, n)) return false;
  const uint64_t kmax = top / d;  // k d <= 2^31 - 1
  std::vector<uint64_t> ks = {1, 2, 3, kmax / 2, kmax > 0 ? kmax - 1 : 0, kmax, kmax + 1};
  for (int i = 0; i < 8; ++i) ks.push_back(kmax ? rnd() % (kmax + 1) : 0);
  for (uint64_t k : ks) {
    if (k == 0) continue;
    if (!check_n(d, f, k * d - 1) || !check_n(d, f, k * d)) return false;
  }
  for (int i = 0; i < 16; ++i)
    if (!check_n(d, f, rnd() >> 33)) return false;
  return true;
}

int sweep() {
  for (unsigned d = 1; d <= 4096; ++d)
    if (!check_d(d)) return 1;
  for (int p = 1; p <= 30; ++p) {
    const unsigned v = 1u << p;
    if (!check_d(v - 1 ? v - 1 : 1) || !check_d(v) || (p < 30 && !check_d(v + 1))) return 1;
  }
  if (!check_d((1u << 30) + 1) || !check_d(0x7fffffffu)) return 1;
  for (int i = 0; i < 4000; ++i) {
    unsigned d = (unsigned)(rnd() >> 33);            // uniform below 2^31
    if (i & 1) d >>= (unsigned)(rnd() % 31);         // and spread over the magnitudes
    if (!check_d(d ? d : 1)) return 1;
  }
  std::printf("ok: %lld fdiv checks\n", checks);
  return 0;
}

std::vector<long long> fields(const std::string& s, std::string* name) {
  std::vector<long long> v;
  std::stringstream ss(s);
  std::string tok;
  bool first = true;
  while (std::getline(ss, tok, ':')) {
    if (first) *name = tok;
    else v.push_back(std::atoll(tok.c_str()));
    first = false;
  }
  return v;
}

long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

int describe(const std::string& c) {
  std::string name;
  const std::vector<long long> a = fields(c, &name);
  auto need = [&](size_t n) { return a.size() == n; };
  if (name == "rms_fwd" && need(2)) {
    std::printf("%s maxc=%d grid=%lld\n", c.c_str(), rw::maxc_for(a[1]), cdiv(a[0], rw::RMS_FWD_WAVES));
  } else if (name == "rms_bwd" && need(3)) {
    const int mc = rw::maxc_for(a[1]), nw = rw::bwd_waves(mc), nb = rw::bwd_blocks(a[0], a[1]);
    std::printf("%s maxc=%d nw=%d full=%d res=%d nb=%d trips=%lld idle_waves=%d ragged=%d\n", c.c_str(), mc, nw,
                a[1] == mc * 512 ? 1 : 0, a[2] ? 1 : 0, nb, cdiv(a[0], (long long)nb * nw), a[0] < (long long)nb * nw,
                a[0] % ((long long)nb * nw) != 0);
  } else if (name == "rms_chain" && need(3)) {
    const int mc = rw::maxc_for(a[1]), nw = rw::bwd_waves(mc), nb = rw::bwd_blocks(a[0], a[1]);
    const long long cpw = rw::chain_cpw(a[2], nb);
    std::printf("%s maxc=%d nw=%d nb=%d cpw=%lld fused=%d\n", c.c_str(), mc, nw, nb, cpw, cpw <= rw::PREV_COLS);
  } else if (name == "ce" && need(2)) {
    std::printf("%s nch=%d\n", c.c_str(), rw::nch_for(a[1], (int)a[0]));
  } else if (name == "swiglu" && need(5)) {
    const bool vec = rw::vec_ok(a[1], a[2], a[3], (const void*)(uintptr_t)a[4], nullptr, nullptr);
    const long long work = vec ? a[0] * a[1] / 8 : a[0] * a[1];
    const int grid = rw::grid_for(work);
    std::printf("%s family=%s grid=%d trips=%lld\n", c.c_str(), vec ? "vec" : "scalar", grid,
                cdiv(work, (long long)grid * 256));
  } else if (name == "rope" && need(4)) {
    const long long total = a[0] * a[1] * a[2] * (a[3] / 16);
    const int grid = rw::rope_grid(total);
    std::printf("%s total=%lld grid=%d trips=%lld\n", c.c_str(), total, grid, cdiv(total, (long long)grid * 256));
  } else if (name == "scale" && need(1)) {
    const int grid = rw::scale_grid(a[0]);
    std::printf("%s grid=%d trips=%lld tail=%lld\n", c.c_str(), grid, cdiv(a[0] / 8, (long long)grid * 256), a[0] % 8);
  } else if (name == "emb" && need(1)) {
    std::printf("%s trips=%lld\n", c.c_str(), cdiv(a[0], rw::EMB_COLS_PER_TRIP));
  } else {
    std::printf("FAIL: bad case %s\n", c.c_str());
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return sweep();
  std::vector<std::string> cases;
  if (std::string(argv[1]) == "-") {
    std::string line;
    while (std::getline(std::cin, line))
      if (!line.empty()) cases.push_back(line);
  } else {
    for (int i = 1; i < argc; ++i) cases.push_back(argv[i]);
  }
  for (const std::string& c : cases)
    if (describe(c)) return 1;
  return 0;
}
