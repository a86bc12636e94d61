// pga_pool.cpp -- the host threads the whole library shares: the pool of persistent helpers behind pool_for, and the janitors that take a call's
// leftovers apart (pga_common.h).
#include "pga_common.h"
#include <atomic>
#include <condition_variable>
#include <deque>
#include <exception>
#include <mutex>
#include <thread>

namespace pga {

// pool_for over a pool of persistent helper threads: a round of a small call runs a dozen of these loops, and starting eight
// std::threads for each costs more than the loop (0.3 ms a time).  The caller always takes part, so a loop makes progress even when
// every helper is busy with the loops of other batches; helpers join a loop through tickets and are counted, the caller leaves only when
// the tickets nobody took are withdrawn and the helpers that joined are done.
namespace {
struct PfJob { std::atomic<size_t> next{0}; size_t n = 0, chunk = 1; void (*run)(void*, size_t) = nullptr; void *ctx = nullptr; int active = 0; std::exception_ptr err; };
struct PfPool {
	std::mutex mu; std::condition_variable cv_work, cv_done; std::deque<PfJob*> tickets; std::vector<std::thread> th; bool stop = false;
	void loop(PfJob *j) { try { for (;;) { const size_t i0 = j->next.fetch_add(j->chunk); if (i0 >= j->n) break; const size_t i1 = std::min(j->n, i0 + j->chunk); for (size_t i = i0; i < i1; ++i) j->run(j->ctx, i); } } catch (...) { std::lock_guard<std::mutex> lk(mu); if (!j->err) j->err = std::current_exception(); j->next.store(j->n); } }
	void worker() {
		std::unique_lock<std::mutex> lk(mu);
		for (;;) {
			cv_work.wait(lk, [&] { return stop || !tickets.empty(); });
			if (stop) return;
			PfJob *j = tickets.front(); tickets.pop_front(); ++j->active;
			lk.unlock(); loop(j); lk.lock();
			if (--j->active == 0) cv_done.notify_all();
		}
	}
	void grow(size_t want) { while (th.size() < want) th.emplace_back([this] { worker(); }); }     // (mu held)
	~PfPool() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv_work.notify_all(); for (auto &t : th) t.join(); }
};
PfPool &pf_pool() { static PfPool *p = new PfPool(); return *p; }       // (leaked on purpose: no destructor order games at exit)
}

void pool_for_raw(size_t n, int n_threads, void (*run)(void*, size_t), void *ctx)
{
	if (n_threads <= 1 || n < 2) { for (size_t i = 0; i < n; ++i) run(ctx, i); return; }
	// (items are taken a few at a time once there are thousands: one shared counter)
	PfJob job; job.n = n; job.chunk = std::max<size_t>(1, n / 256); job.ctx = ctx; job.run = run;
	const size_t helpers = std::min<size_t>((size_t)n_threads - 1, n - 1);
	PfPool &P = pf_pool();
	{
		std::lock_guard<std::mutex> lk(P.mu);
		P.grow(std::min<size_t>(64, std::max<size_t>(P.th.size(), (size_t)std::max(usable_cpus(), n_threads))));
		for (size_t h = 0; h < helpers; ++h) P.tickets.push_back(&job);
	}
	P.cv_work.notify_all();
	P.loop(&job);
	{
		std::unique_lock<std::mutex> lk(P.mu);
		for (auto it = P.tickets.begin(); it != P.tickets.end();) it = *it == &job ? P.tickets.erase(it) : it + 1;
		P.cv_done.wait(lk, [&] { return job.active == 0; });
	}
	if (job.err) std::rethrow_exception(job.err);
}

// a detached thread that destroys what it is handed, one object after the other (leaked on purpose, like the pool)
struct Janitor {
	struct Item { void *obj; void (*destroy)(void*); };
	std::mutex mu; std::condition_variable cv; std::deque<Item> q; std::thread th;
	Janitor() : th([this] { for (;;) { Item it; { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !q.empty(); }); it = q.front(); q.pop_front(); } it.destroy(it.obj); } }) { th.detach(); }
};
Janitor *janitor_start() { return new Janitor(); }
void janitor_take(Janitor *J, void *obj, void (*destroy)(void*))
{
	{ std::lock_guard<std::mutex> lk(J->mu); J->q.push_back(Janitor::Item{obj, destroy}); }
	J->cv.notify_one();
}

} // namespace pga
