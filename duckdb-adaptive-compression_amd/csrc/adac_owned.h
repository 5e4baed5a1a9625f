// adac_owned.h — who frees what: the one owner type behind every device buffer, pinned host word and event that a
// layout, a plan or an entry point holds (adac_capi.cpp).  Pure host code, no HIP: the memory calls are two functions
// this header only declares — adac_capi.cpp defines them over the HIP runtime, tests/owned_groups_check.cpp over a
// counting allocator that fails on demand.
//
// The rule: buffers that are only useful together are allocated as a GROUP, all or nothing (alloc_group), and a group
// that must be cleared or uploaded before its first use is built in locals and moved into its object only after those
// enqueues were accepted.  An object therefore holds a group complete and initialised, or not at all.
#pragma once

#include <stddef.h>

#include <utility>

namespace adac {

enum class Mem { Device, Pinned, Event };

// 0, or the runtime's error code.  `bytes` is 0 for an event, whose handle is written through `p` as if it were a
// void * (the runtime's event type is a pointer to an opaque struct).  owned_free is never called with a null pointer.
int owned_alloc(Mem kind, void **p, size_t bytes);
int owned_free(Mem kind, void *p);

// Move-only owner of `n` elements of T (of one event when K is Mem::Event, whose T is the runtime's opaque struct).
// Converts to the bare pointer, which is what the launchers take.  Mind what that also lets compile: a free or a
// delete of an owner, and arithmetic on it, go through the same conversion — the pointer stays the owner's.
template <class T, Mem K = Mem::Device>
class Owned {
public:
	Owned() = default;
	Owned(const Owned &) = delete;
	Owned &operator=(const Owned &) = delete;
	Owned(Owned &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
	Owned &operator=(Owned &&o) noexcept {
		if (this != &o) {
			reset();
			p_ = o.p_, n_ = o.n_;
			o.p_ = nullptr, o.n_ = 0;
		}
		return *this;
	}
	~Owned() { reset(); }

	void reset() {
		if (p_) (void)owned_free(K, p_);
		p_ = nullptr, n_ = 0;
	}
	// A fresh array of n elements in place of the current one, which stays if the allocation fails.  n == 0 still
	// yields one element: the kernels are handed these pointers for empty layouts too.
	int alloc(size_t n) {
		void *q = nullptr;
		const int e = owned_alloc(K, &q, bytes_of(n));
		if (e != 0) return e;
		reset();
		p_ = static_cast<T *>(q), n_ = n;
		return 0;
	}
	T *get() const { return p_; }
	operator T *() const { return p_; }
	size_t size() const { return n_; } // elements asked for, which may be 0
	// Bytes ALLOCATED, never 0: what a clear covers.  As the length of an upload of size() elements it is right only
	// where size() != 0, and every such copy stands under that test.
	size_t bytes() const { return bytes_of(n_); }

private:
	static size_t bytes_of(size_t n) {
		if constexpr (K == Mem::Event) return 0;
		else return (n ? n : 1) * sizeof(T);
	}
	T *p_ = nullptr;
	size_t n_ = 0;
};

template <class T>
using DeviceArray = Owned<T, Mem::Device>;

// alloc_group(a, na, b, nb, ...): every owner gets its array, or none changes and the first error comes back.  (Each
// level keeps its fresh array in a local until the levels below have succeeded.)
inline int alloc_group() { return 0; }
template <class O, class... Rest>
int alloc_group(O &owner, size_t n, Rest &&...rest) {
	O fresh;
	int e = fresh.alloc(n);
	if (e == 0) e = alloc_group(std::forward<Rest>(rest)...);
	if (e == 0) owner = std::move(fresh);
	return e;
}

// The lazily allocated groups: nothing to do when the group is there (its first member speaks for all of them).
template <class O, class... Rest>
int ensure_group(O &first, size_t n, Rest &&...rest) {
	return first ? 0 : alloc_group(first, n, std::forward<Rest>(rest)...);
}

} // namespace adac
