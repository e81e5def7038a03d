// orbfe_shim.h -- what the shim translation units share: the status check that throws, the per-thread grow-only handle, and the
// queue of rand() draws of the two RANSAC solvers.  Everything has internal linkage: each translation unit that includes this
// has its own handle and its own queue (the Sim3 and the PnP solver each give back to, and take from, their own).
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbfe.h"

namespace orbfe_shim
{
namespace
{
inline void check(orbfe_status s, const char *what)
{
    if (s != ORBFE_OK) throw std::runtime_error(std::string(what) + ": " + orbfe_strerror(s) + " (" + orbfe_last_error() + ")");
}

// owns a handle until its thread ends
template <class H, void (*Destroy)(H *)>
struct Holder {
    H *h = nullptr;
    int cap = 0;
    ~Holder() { Destroy(h); }
};

// one handle per thread, grown to the largest count seen
template <class H, orbfe_status (*Create)(int32_t, int32_t, int32_t, H **), void (*Destroy)(H *)>
H *handle_for(int n, const char *create_name)
{
    static thread_local Holder<H, Destroy> hold;
    if (!hold.h || n > hold.cap) {
        Destroy(hold.h);
        hold.h = nullptr;
        const int cap = n > 4096 ? n : 4096;
        check(Create(-1, cap, 1, &hold.h), create_name);
        hold.cap = cap;
    }
    return hold.h;
}

// draws handed to a call that it did not use, oldest first
inline std::deque<int32_t> &pending()
{
    static thread_local std::deque<int32_t> q;
    return q;
}

// k draws: the pending ones first, then rand()
inline std::vector<int32_t> take_draws(size_t k)
{
    std::deque<int32_t> &q = pending();
    std::vector<int32_t> draws(k);
    for (size_t i = 0; i < k; i++) {
        if (!q.empty()) {
            draws[i] = q.front();
            q.pop_front();
        } else {
            draws[i] = (int32_t)rand();
        }
    }
    return draws;
}

// all but the first `used` go back to the front of the queue
inline void give_back(const std::vector<int32_t> &draws, size_t used)
{
    for (size_t k = draws.size(); k > used; k--) pending().push_front(draws[k - 1]);
}
}  // namespace
}  // namespace orbfe_shim
