// gicp_lockstep.hpp -- the rendezvous behind mi355ndt_gicp_batch_align: n independent optimisers, one worker thread each, advance in lockstep
// so that ONE evaluation serves every slot that is waiting for one.
//
//   worker k      runs its slot's loop as the single-pair surface does; where that loop would evaluate on the device it calls
//                 post(k, request, &record) and blocks until the record is there; it ends by returning from its body.
//   coordinator   (the calling thread, run()) waits until every unfinished slot has posted or ended, hands all posted requests to
//                 serve(slots, n, requests, records) -- both arrays indexed by slot, slots[0 .. n) ascending --, releases the slots and waits again.
//                 That is one round; the rounds end when no slot is left.
//   failure       serve returns false: nothing is served any more.  The posted slots and every later post get a zero record and `false` at
//                 once, so each worker runs out through its own budgets; run() joins every worker before it returns false.
// rounds() counts the calls of serve, requests(k) the posts of slot k: every live slot posts once per round, so rounds = max_k requests(k).
// Nothing of HIP in this file: it compiles into the library's host side and into tests/cpp/gicp_lockstep_main.cpp.  Workers touch their own
// request and record only; everything shared is read and written under the one mutex.
#pragma once
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace gicp_lockstep {

template <typename Req, typename Rec>
class Lockstep {
 public:
  explicit Lockstep(int n) : n_(n), st_((size_t)n, DONE), req_((size_t)n), rec_((size_t)n), requests_((size_t)n, 0) {}

  // worker k: one request; false (and a zero record) once an evaluation has failed
  bool post(int k, const Req& r, Rec* out) {
    std::unique_lock<std::mutex> l(mu_);
    requests_[(size_t)k]++;
    if (failed_) { *out = Rec{}; return false; }
    req_[(size_t)k] = r;
    st_[(size_t)k] = POSTED;
    if (--computing_ == 0) cv_coord_.notify_one();
    cv_work_.wait(l, [&] { return st_[(size_t)k] == COMPUTING; });
    *out = rec_[(size_t)k];
    return !failed_;
  }

  // body(k) on a thread per slot, the rounds on the calling thread; returns false when serve failed (or a thread could not be started)
  template <typename Body, typename Serve>
  bool run(Body body, Serve serve) {
    std::vector<std::thread> workers;
    {
      std::lock_guard<std::mutex> l(mu_);
      for (int k = 0; k < n_; k++) st_[(size_t)k] = COMPUTING;
      computing_ = n_;
    }
    for (int k = 0; k < n_; k++) {
      try {
        workers.emplace_back([this, body, k] { body(k); done(k); });
      } catch (...) {                              // no thread for slot k .. n - 1: they end here, the started ones run out
        std::lock_guard<std::mutex> l(mu_);
        failed_ = true;
        for (int j = k; j < n_; j++) st_[(size_t)j] = DONE;
        computing_ -= n_ - k;
        break;
      }
    }
    std::vector<int> slots((size_t)n_);
    for (;;) {
      std::unique_lock<std::mutex> l(mu_);
      cv_coord_.wait(l, [&] { return computing_ == 0; });
      int n = 0;
      for (int k = 0; k < n_; k++)
        if (st_[(size_t)k] == POSTED) slots[(size_t)n++] = k;
      if (n == 0) break;
      bool ok = !failed_;
      if (ok) {
        rounds_++;
        l.unlock();                                // (every posted worker is blocked: its request and record are the coordinator's for now)
        ok = serve(slots.data(), n, req_.data(), rec_.data());
        l.lock();
      }
      if (!ok) {
        failed_ = true;
        for (int j = 0; j < n; j++) rec_[(size_t)slots[(size_t)j]] = Rec{};
      }
      for (int j = 0; j < n; j++) st_[(size_t)slots[(size_t)j]] = COMPUTING;
      computing_ += n;
      cv_work_.notify_all();
    }
    for (auto& w : workers) w.join();
    return !failed_;
  }

  int rounds() const { return rounds_; }
  int requests(int k) const { return requests_[(size_t)k]; }

 private:
  enum State { COMPUTING, POSTED, DONE };
  void done(int k) {
    std::lock_guard<std::mutex> l(mu_);
    st_[(size_t)k] = DONE;
    if (--computing_ == 0) cv_coord_.notify_one();
  }
  const int n_;
  std::mutex mu_;
  std::condition_variable cv_coord_, cv_work_;
  std::vector<State> st_;
  std::vector<Req> req_;
  std::vector<Rec> rec_;
  std::vector<int> requests_;
  int computing_ = 0, rounds_ = 0;
  bool failed_ = false;
};

}  // namespace gicp_lockstep
