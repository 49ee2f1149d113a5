// host_pool_main.cpp - the thread pool of the host-parallel routines (csrc/host_parallel.hpp) on its own: regions whose
// body throws on a worker only, on the calling thread only, and on every thread, at 1, 2 and 8 threads.  Each time
// exactly one exception reaches the caller, no body is still running by then, and the pool runs the next region
// correctly.  One line per case, exit status 0 when all hold.  (Built and run by tests/test_face_table_cpu.py, and under
// AddressSanitizer / ThreadSanitizer by tools/sanitize_host.sh.)
//   g++ -O2 -std=c++17 -pthread -Iflooder_amd/csrc tests/host_pool_main.cpp -o host_pool_main
#include "host_parallel.hpp"

#include <chrono>
#include <cstdio>
#include <stdexcept>

namespace {

enum Who { WORKER_ONLY, CALLER_ONLY, ALL_THREADS };
const char* const WHO[] = {"worker", "caller", "all"};

bool throws(Who who, int tid, int nt) {
  if (who == ALL_THREADS) return true;
  if (who == CALLER_ONLY) return tid == 0;
  return nt == 1 ? false : tid == nt - 1;      // (one thread has no worker: the region then ends without an exception)
}

// sum of 0 .. n-1 over an ordinary parallel_for
bool sums_correctly(Pool& pool) {
  const int64_t n = 1000000;
  std::atomic<int64_t> total{0};
  pool.parallel_for(n, 1 << 12, [&](int64_t a, int64_t b, int) {
    int64_t s = 0;
    for (int64_t i = a; i < b; ++i) s += i;
    total.fetch_add(s, std::memory_order_relaxed);
  });
  return total.load() == n * (n - 1) / 2;
}

bool one_case(int nt, Who who, bool through_parallel_for) {
  Pool pool(nt);
  bool ok = true;
  for (int round = 0; round < 3; ++round) {      // (the pool is used again after every failed region)
    std::atomic<int> running{0}, entered{0};
    int caught = 0, running_at_catch = -1;
    const int expect = (who == WORKER_ONLY && nt == 1) ? 0 : 1;
    auto body = [&](int tid) {
      running.fetch_add(1);
      entered.fetch_add(1);
      struct Leave {
        std::atomic<int>& r;
        ~Leave() { r.fetch_sub(1); }
      } leave{running};
      // the threads that do not throw are still at work when the exception is raised
      if (!throws(who, tid, nt)) std::this_thread::sleep_for(std::chrono::milliseconds(20));
      else throw std::runtime_error("thrown inside a parallel region");
    };
    try {
      if (through_parallel_for) {
        // one item per chunk, handed out in turn: the item number stands for the thread of the plain region, and a
        // thread that throws takes no further item
        pool.parallel_for(nt, 1, [&](int64_t a, int64_t, int) { body((int)a); });
      } else {
        pool.run(body);
      }
    } catch (const std::runtime_error&) {
      ++caught;
      running_at_catch = running.load();
    }
    if (caught == 0) running_at_catch = running.load();
    ok = ok && caught == expect && running_at_catch == 0 && entered.load() == nt && sums_correctly(pool);
  }
  std::printf("threads %d, throws on %-6s, %-12s: %s\n", nt, WHO[who], through_parallel_for ? "parallel_for" : "run",
              ok ? "ok" : "FAILED");
  return ok;
}

}  // namespace

int main() {
  bool ok = true;
  for (int nt : {1, 2, 8})
    for (Who who : {WORKER_ONLY, CALLER_ONLY, ALL_THREADS})
      for (bool pf : {false, true}) ok = one_case(nt, who, pf) && ok;
  std::printf("%s\n", ok ? "all ok" : "FAILED");
  return ok ? 0 : 1;
}
