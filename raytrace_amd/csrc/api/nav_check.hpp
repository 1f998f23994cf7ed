// nav_check.hpp — the host half of the navigation fields (rt_nav_*) that needs no context: the store of live fields, the verdict on
// a build's and a sample's plain arguments, the box test, and the launch plan of a build — tiles, level launches and the words of
// the device scratch.  Plain C++ with no HIP include, so that tests/nav_field_main.cpp runs this very code on the CPU.  Everything
// is integer arithmetic (include/rt_abi.h "Navigation fields").
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/rt_abi.h"

namespace rta __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxNavFields = 64;         // live fields per context
constexpr int32_t kMaxNavExtent = 256;         // per axis
constexpr uint32_t kMaxNavDist = 4096;         // RtNavBuild.max_dist
constexpr uint32_t kMaxNavGoals = 4096;        // goals per build
constexpr uint32_t kMaxNavAgents = 1u << 20;   // agents per sample
constexpr uint32_t kNavTile = 16;              // a workgroup of the level kernel owns 16 x 16 columns
constexpr uint32_t kNavLevels = 8;             // G: levels per launch (RT_NAV_LEVELS chooses 1 or 4 for A/B timing)
// the scratch's head, in words: word j (1..4097) says whether level launch j has a frontier to start from, word kNavTruncWord
// whether a cell lies at max_dist + 1, words kNavSpareResult.. are a spare RtNavResult
constexpr size_t kNavHeadWords = 4112, kNavTruncWord = 4100, kNavSpareResult = 4104;

// ---- the store: ids are serial << 6 | slot with serial >= 1, so that an id is never 0 and a destroyed id stays unknown ------------
struct NavEntry {
    uint32_t id = 0;             // 0: the slot is free
    int32_t ext[3] = {0, 0, 0};
    int32_t lo[3] = {0, 0, 0};   // of the build enqueued last
    bool built = false;          // a build was enqueued
    bool used = false;           // a build or sample that names it may still be running
    uint64_t block = 0;          // device address: the scratch (nav_scratch_words), then dist u16[ez][ey][ex], then move u8[ez][ey][ex]
    size_t cells() const { return (size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2]; }
};
struct NavStore {
    std::vector<NavEntry> slots;
    uint32_t live = 0, serial = 0;
    uint32_t levels = kNavLevels;   // G of this context's builds
    NavEntry* find(uint32_t id) {
        const uint32_t s = id & (kMaxNavFields - 1u);
        return id != 0u && s < slots.size() && slots[s].id == id ? &slots[s] : nullptr;
    }
    // a new entry with an id of its own, or null when kMaxNavFields are live
    NavEntry* add(const int32_t ext[3]) {
        if (live == kMaxNavFields) return nullptr;
        uint32_t s = 0;
        while (s < slots.size() && slots[s].id != 0u) s++;
        if (s == slots.size()) slots.emplace_back();
        serial = serial >= (1u << 26) - 1u ? 1u : serial + 1u;
        NavEntry& e = slots[s];
        e = NavEntry{};
        e.id = (serial << 6) | s;
        for (int k = 0; k < 3; k++) e.ext[k] = ext[k];
        live++;
        return &e;
    }
    void remove(NavEntry* e) { *e = NavEntry{}; live--; }
};

inline bool nav_extent_valid(const int32_t ext[3]) {
    for (int k = 0; k < 3; k++)
        if (ext[k] < 1 || ext[k] > kMaxNavExtent) return false;
    return true;
}

// What is wrong with a build's arguments apart from the id and the box, or nullptr.
inline const char* nav_build_error(const RtNavBuild* p, const RtNavGoal* goals, uint32_t goal_count) {
    if (!p) return "null params";
    if (p->max_dist < 1u || p->max_dist > kMaxNavDist) return "max_dist must be 1..4096";
    if (p->height < 1u || p->height > 4u) return "height must be 1..4";
    if (p->max_climb > 2u) return "max_climb must be 0..2";
    if (p->max_drop > 8u) return "max_drop must be 0..8";
    if (p->goal_snap > 8u) return "goal_snap must be 0..8";
    if (p->reserved[0] != 0u || p->reserved[1] != 0u || p->reserved[2] != 0u) return "a reserved word is not 0";
    if (goal_count > kMaxNavGoals) return "more than 4096 goals";
    if (goal_count > 0u && !goals) return "null goals";
    return nullptr;
}

// The box [lo, lo + ext) lies inside [0, 2^logr)^3.
inline bool nav_box_inside(const int32_t lo[3], const int32_t ext[3], int logr) {
    const int32_t R = (int32_t)1 << logr;
    for (int k = 0; k < 3; k++)
        if (lo[k] < 0 || ext[k] > R - lo[k]) return false;
    return true;
}

// What is wrong with a sample's plain arguments, or nullptr (count == 0 needs no pointers).
inline const char* nav_sample_error(const void* agents, uint32_t count, const void* steps) {
    if (count > kMaxNavAgents) return "more than 2^20 agents in one call";
    if (count > 0u && (!agents || !steps)) return "null pointer";
    return nullptr;
}

// ---- the plan of a field and of a build ------------------------------------------------------------------------------------------
// The bitmaps hold a row of bits along x per (y, z), in 16-bit pieces (one per tile along x), `row_halves` of them per row — the
// tiles along x rounded up to an even number, so that a row is whole dwords.  Five bitmaps follow the head: the unoccupied bits, and
// two ping-pong pairs (unreached standable cells, frontier).
struct NavPlan {
    uint32_t tiles_x = 0, tiles_y = 0, tiles = 0;   // workgroups of a level launch
    uint32_t row_halves = 0;
    size_t bitmap_words = 0;                        // of one bitmap
    size_t scratch_words = 0;                       // head + five bitmaps
    size_t block_bytes = 0;                         // scratch, dist and move: what rt_nav_create allocates
    uint32_t launches = 0;                          // level launches of a build (0 without max_dist)
};

// `levels`: G; max_dist 0 plans the field alone
inline NavPlan nav_plan(const int32_t ext[3], uint32_t max_dist, uint32_t levels) {
    NavPlan p;
    p.tiles_x = ((uint32_t)ext[0] + kNavTile - 1u) / kNavTile;
    p.tiles_y = ((uint32_t)ext[1] + kNavTile - 1u) / kNavTile;
    p.tiles = p.tiles_x * p.tiles_y;
    p.row_halves = (p.tiles_x + 1u) & ~1u;
    p.bitmap_words = (size_t)ext[1] * (size_t)ext[2] * (size_t)(p.row_halves / 2u);
    p.scratch_words = kNavHeadWords + 5u * p.bitmap_words;
    const size_t cells = (size_t)ext[0] * (size_t)ext[1] * (size_t)ext[2];
    p.block_bytes = p.scratch_words * 4u + cells * 3u;
    // levels 1 .. max_dist are written, level max_dist + 1 is only looked at (RtNavResult.truncated): G levels per launch
    p.launches = max_dist == 0u ? 0u : (max_dist + 1u + levels - 1u) / levels;
    return p;
}

}  // namespace rta
