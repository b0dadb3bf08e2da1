// rmx_track.h -- the term table of a tracking objective (rmx_adjoint_track): one pure function from the caller's terms to what the
// kernels read.  Host only and free of HIP types, in the manner of rmx_select.h (tests/test_adjoint_track_host.py compiles it with
// plain g++ behind tests/trackplan/track_plan_shim.cpp).
#pragma once
#include <string>
#include <vector>

#include "redmax_hip.h"   /* rmx_track_term: a term as the caller lists it (plain C) */

namespace rmx_track {

// One term as the kernels read it.
struct DevTerm {
    double xl[3];
    double wpos;
    int node;      // device node of the body
    int orig;      // the term's position in the caller's array: row of the target table
};
static_assert(sizeof(DevTerm) == 40, "DevTerm: four doubles and two ints, no padding");

struct Plan {
    std::string error;             // empty: the plan holds
    std::vector<DevTerm> terms;    // sorted by step; terms of one step in the caller's order
    std::vector<int> begin;        // [nsteps + 1]: step k owns terms begin[k-1] .. begin[k]-1
};

inline Plan plan_terms(const rmx_track_term* terms, const int nterms, const int nsteps, const int nlist, const int* node_of_listing) {
    Plan p;
    if (!terms) { p.error = "null terms"; return p; }
    if (nterms < 1) { p.error = "nterms < 1"; return p; }
    if (nsteps < 1) { p.error = "nsteps < 1"; return p; }
    for (int i = 0; i < nterms; ++i) {
        if (terms[i].body < 0 || terms[i].body >= nlist) {
            p.error = "term " + std::to_string(i) + ": body " + std::to_string(terms[i].body) + " is outside the listing of " +
                      std::to_string(nlist) + " bodies";
            return p;
        }
        if (terms[i].step < 1 || terms[i].step > nsteps) {
            p.error = "term " + std::to_string(i) + ": step " + std::to_string(terms[i].step) + " is outside [1, " + std::to_string(nsteps) + "]";
            return p;
        }
    }
    // counting sort by step: stable, so the terms of one step keep the caller's order
    p.begin.assign((size_t)nsteps + 1, 0);
    for (int i = 0; i < nterms; ++i) ++p.begin[(size_t)terms[i].step];
    for (int k = 1; k <= nsteps; ++k) p.begin[(size_t)k] += p.begin[(size_t)k - 1];
    std::vector<int> at(p.begin.begin(), p.begin.end() - 1);
    p.terms.resize((size_t)nterms);
    for (int i = 0; i < nterms; ++i) {
        DevTerm& d = p.terms[(size_t)at[(size_t)terms[i].step - 1]++];
        for (int c = 0; c < 3; ++c) d.xl[c] = terms[i].xlocal[c];
        d.wpos = terms[i].wpos;
        d.node = node_of_listing[terms[i].body];
        d.orig = i;
    }
    return p;
}

}      // namespace rmx_track
