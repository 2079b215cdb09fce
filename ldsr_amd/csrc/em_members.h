// em_members.h -- THE list of compiled members of the two EM kernel families.  One entry = one translation
// unit (em_scan_<L>_<W>.o / em_pair_<L>_<LPC>.o, compiled from em_scan_launch.inc / em_pair_launch.inc with the
// entry's two numbers as -D flags).  Everything else is derived from this file and from nothing else: the
// Makefile's object list (it greps the SCAN(..) / PAIR(..) entries below), the launchers' dispatch, the chunk
// lengths the plans choose from and the kernel inventory (kernels_scan.hip).  Which variants of a member exist
// per padded (PP, QQ) is scan_variant() / pair_variant() (em_scan_impl.h, em_pair_impl.h).
// Adding or dropping a member is an edit of one entry here.  Within a W / an LPC the entries are in ascending
// order of L: the plans take the first chunk length that fits (static_assert below).
#pragma once

// scan family: SCAN(chunk length L, waves per cell W)
#define LDSR_SCAN_MEMBERS(SCAN) \
    SCAN(2, 1) SCAN(3, 1) SCAN(4, 1) SCAN(6, 1) SCAN(8, 1) SCAN(10, 1) SCAN(12, 1) SCAN(13, 1) \
    SCAN(14, 1) SCAN(15, 1) SCAN(16, 1) SCAN(20, 1) SCAN(24, 1) SCAN(28, 1) SCAN(32, 1) \
    SCAN(20, 2) SCAN(24, 2) SCAN(28, 2) SCAN(32, 2) \
    SCAN(20, 4) SCAN(24, 4) SCAN(28, 4) SCAN(32, 4)

// pair family: PAIR(chunk length L, lanes per cell LPC) -- 32: two cells per wave, 16: four
#define LDSR_PAIR_MEMBERS(PAIR) \
    PAIR(3, 32) PAIR(4, 32) PAIR(5, 32) PAIR(6, 32) PAIR(7, 32) PAIR(8, 32) PAIR(9, 32) PAIR(10, 32) \
    PAIR(11, 32) PAIR(12, 32) PAIR(13, 32) PAIR(14, 32) PAIR(15, 32) PAIR(16, 32) PAIR(17, 32) PAIR(18, 32) \
    PAIR(19, 32) PAIR(20, 32) PAIR(21, 32) PAIR(22, 32) PAIR(23, 32) PAIR(24, 32) PAIR(25, 32) PAIR(26, 32) \
    PAIR(27, 32) PAIR(28, 32) PAIR(29, 32) PAIR(30, 32) PAIR(31, 32) PAIR(32, 32) \
    PAIR(5, 16) PAIR(6, 16) PAIR(7, 16) PAIR(8, 16) PAIR(9, 16) PAIR(10, 16) PAIR(11, 16) PAIR(12, 16) \
    PAIR(13, 16) PAIR(14, 16) PAIR(15, 16) PAIR(16, 16) PAIR(17, 16) PAIR(18, 16) PAIR(19, 16) PAIR(20, 16) \
    PAIR(21, 16) PAIR(22, 16) PAIR(23, 16) PAIR(24, 16) PAIR(25, 16) PAIR(26, 16) PAIR(27, 16) PAIR(28, 16) \
    PAIR(29, 16) PAIR(30, 16) PAIR(31, 16) PAIR(32, 16)

struct EmMember { int L, n; };      // n: W (scan) or LPC (pair)
#define LDSR_MEMBER_ENTRY(L, n) {L, n},
static constexpr EmMember kScanMembers[] = {LDSR_SCAN_MEMBERS(LDSR_MEMBER_ENTRY)};
static constexpr EmMember kPairMembers[] = {LDSR_PAIR_MEMBERS(LDSR_MEMBER_ENTRY)};
#undef LDSR_MEMBER_ENTRY
// the plans' search order: ascending L among the entries with the same n
template <int N>
constexpr bool members_ascend(const EmMember (&m)[N]) {
    for (int i = 0; i < N; i++)
        for (int k = i + 1; k < N; k++)
            if (m[k].n == m[i].n && m[k].L <= m[i].L) return false;
    return true;
}
static_assert(members_ascend(kScanMembers) && members_ascend(kPairMembers), "em_members.h: ascending L per W / LPC");
