// lmi_filter_plan.h -- the host arithmetic of a filter set (lmi_filter_create, lmi_*_union_filtered; include/lmi_hip.h): the argument
// checks, the normal form of the id lists and the check of a batch's filter_of.  Pure host code: the standard library only, no HIP, so
// that tests/host/filter_plan_selftest.cpp can run it under the sanitizers on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace lmi_filter_plan {

constexpr int MAX_FILTERS = 1024;          // nf of a filter set
constexpr int64_t MAX_IDS = 1ll << 31;     // offsets[nf] stays below it: positions in the concatenated lists are 32-bit on the device
constexpr int KEEP = 0, DROP = 1;          // LMI_FILTER_KEEP, LMI_FILTER_DROP

// Why lmi_filter_create refuses its lists, or nullptr.  bad (nullable) <- the filter the message is about (-1: none).
inline const char* check_lists(const uint32_t* ids, const int64_t* offsets, int nf, const int32_t* modes, int* bad) {
    if (bad) *bad = -1;
    if (nf < 1 || nf > MAX_FILTERS) return "nf outside [1,1024]";
    if (!offsets || !modes) return "offsets and modes must not be NULL";
    if (offsets[0] != 0) return "offsets[0] is not 0";
    for (int j = 0; j < nf; ++j) {
        if (bad) *bad = j;
        if (offsets[j + 1] < offsets[j]) return "the offsets are not non-decreasing";
        if (offsets[j + 1] >= MAX_IDS) return "2^31 ids or more in all";
        if (modes[j] != KEEP && modes[j] != DROP) return "a mode is neither LMI_FILTER_KEEP (0) nor LMI_FILTER_DROP (1)";
    }
    if (bad) *bad = -1;
    if (offsets[nf] > 0 && !ids) return "ids must not be NULL where a list holds ids";
    return nullptr;
}

// The normal form: every list sorted ascending and without duplicates (one that arrives so is only checked), the lists back to back.
// ids [off[nf]], off [nf + 1]; off[nf] <= offsets[nf] < 2^31.
struct Lists {
    std::vector<uint32_t> ids;
    std::vector<int32_t> off;
};
inline Lists normalise(const uint32_t* ids, const int64_t* offsets, int nf) {
    Lists out;
    out.off.assign((size_t)nf + 1, 0);
    out.ids.reserve((size_t)offsets[nf]);
    std::vector<uint32_t> one;
    for (int j = 0; j < nf; ++j) {
        const int64_t n = offsets[j + 1] - offsets[j];
        if (n > 0) {
            one.assign(ids + offsets[j], ids + offsets[j + 1]);
            if (!std::is_sorted(one.begin(), one.end())) std::sort(one.begin(), one.end());
            one.erase(std::unique(one.begin(), one.end()), one.end());
            out.ids.insert(out.ids.end(), one.begin(), one.end());
        }
        out.off[(size_t)j + 1] = (int32_t)out.ids.size();
    }
    return out;
}

// whether id is allowed by the normalised list j under mode (what filter_mark_kernel computes per row)
inline bool allows(const Lists& l, int j, int mode, uint32_t id) {
    const bool hit = std::binary_search(l.ids.begin() + l.off[(size_t)j], l.ids.begin() + l.off[(size_t)j + 1], id);
    return mode == DROP ? !hit : hit;
}

// The first query whose filter_of lies outside [-1, nf), or -1.  filter_of == nullptr: every query uses filter 0.
inline int64_t first_bad_filter_of(const int32_t* filter_of, int64_t nq, int nf) {
    if (!filter_of) return -1;
    for (int64_t q = 0; q < nq; ++q)
        if (filter_of[q] < -1 || filter_of[q] >= nf) return q;
    return -1;
}

// the words of one filter's mask row: one per row-block of the slab
inline int64_t mask_words(int nf, int64_t n_rb_total) { return (int64_t)nf * n_rb_total; }
// where row r of a bucket that starts at row-block rb_start lies in filter j's mask: (word, bit)
inline int64_t mask_word(int j, int64_t n_rb_total, int64_t rb_start, int64_t r) { return (int64_t)j * n_rb_total + rb_start + (r >> 5); }
inline int mask_bit(int64_t r) { return (int)(r & 31); }

}  // namespace lmi_filter_plan
