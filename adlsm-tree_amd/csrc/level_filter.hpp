// adlsm-tree_amd/csrc/level_filter.hpp -- the filter stage of the reference's
// point-lookup path, batched: many lookups against every candidate SSTable of
// a level in ONE device launch.
//
// Reference path per key (src/db.cpp:164-197 -> Revision::Get ->
// Level::Get, src/revision.cpp:265-310): walk files_meta_ newest first, skip
// a table whose [min_inner_key, max_inner_key] range does not cover the
// lookup key (:279-287), open its reader from the table cache
// (DB::GetSSTableReader, src/db.cpp:340-364) and call SSTableReader::Get,
// whose first step is the bloom check FilterBlockReader::IsKeyExists(0,
// user_key) (src/sstable.cpp:238): NOT_FOUND without touching the index or
// data blocks when the filter says the key is absent.
//
// Here the same candidate tables are chosen for every key of a batch (same
// comparison, same visiting order), all (key, table) pairs go to the
// FilterCache in one probe launch, and the caller gets, per key, its
// candidates in Level::Get's order with the filter's answer for each -- the
// tables it still has to read.
#pragma once
#include <stdint.h>

#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <vector>

#include "filter_block.hpp"
#include "rc.hpp"

struct adl_bloom_level;
struct adl_bloom_revision;
namespace adl_level {
struct Index;
}

namespace adl {

using namespace std;

/* One SSTable of a level as Level::Get sees it: the oid it is cached under
 * (sha256 hex, src/revision.cpp:290) and FileMetaData's key range
 * (src/file_util.hpp:157-158), as inner keys: user_key + LE64 seq + op byte
 * (src/keys.cpp:76-84). */
struct TableRange {
  string oid;
  string min_inner_key;
  string max_inner_key;
};

/* inner key a < inner key b as MemKey::operator< on the decoded keys */
bool InnerKeyLess(string_view a, string_view b);
/* MemKey(user_key, seq, OP_PUT) < inner key k, as MemKey::operator<
 * (src/keys.cpp:61-74): user keys ascending, then seq descending, then op
 * descending. */
bool LookupLess(string_view user_key, int64_t seq, string_view inner_key);
/* inner key k < MemKey(user_key, seq, OP_PUT) */
bool InnerLessLookup(string_view inner_key, string_view user_key, int64_t seq);

/* Level::Get's range test (src/revision.cpp:281-287): true when the table
 * must be visited for (user_key, seq). */
bool TableCoversKey(const TableRange &t, string_view user_key, int64_t seq);

struct MultiGetFilterResult {
  vector<uint32_t> begin;  /* key i's candidates: [begin[i], begin[i+1]) */
  vector<uint32_t> table;  /* index into `tables`, in Level::Get's visiting order */
  vector<uint8_t> maybe;   /* the filter's answer; 0 = NOT_FOUND for that table */
  uint64_t uncached = 0;   /* pairs whose table was not in the cache (answered 1) */
};

/* tables: the level's SSTables, any order; they are visited as Level::Get
 * walks files_meta_ -- a set ordered by min_inner_key (FileMetaData::operator<,
 * src/file_util.hpp:163-165) iterated in reverse (src/revision.cpp:278).
 * user_keys: the batch; seq: the lookup's sequence (DB::Get reads
 * sequence_id_, src/db.cpp:168).  One cache probe for all pairs: each key
 * is handed over once with its candidate list (FilterCache::ProbeFanout)
 * where that saves upload, otherwise one query per pair (FilterCache::Probe);
 * the answers are the same.  ADL_BLOOM_LEVEL_FANOUT=0 / 2 forces the pair /
 * the fan-out path. */
/* The candidate selection of LevelMultiGetFilter alone (host only): key i's
 * candidate tables are table[begin[i] .. begin[i+1]), in visiting order. */
void LevelCandidates(const vector<TableRange> &tables, const vector<string_view> &user_keys, int64_t seq,
                     vector<uint32_t> &begin, vector<uint32_t> &table);

RC LevelMultiGetFilter(FilterCache &cache, const vector<TableRange> &tables, const vector<string_view> &user_keys,
                       int64_t seq, MultiGetFilterResult &out);

/* A level described ONCE, where its revision installs it, and asked about many
 * times: the region index LevelCandidates builds per call (boundary user
 * keys, per region the candidate tables in visiting order; see
 * level_index_core.hpp), kept on the host and -- from the first device
 * multi-get on, as an adl_bloom_level of the C-ABI -- on the device.  It does
 * not depend on a lookup's seq.  Immutable, so any number of threads may look
 * keys up in it at once.  Drop it with the revision.
 *
 * Host memory: the index, plus a copy of the tables' oids and ranges.  The
 * C-ABI library is a separate one and its level handle is opaque, so the first
 * device batch builds a second index inside that handle (another 0.7-1 ms for
 * 2 000 tables, once) and the level's host footprint doubles from then on; a
 * level whose batches all stay below the threshold never pays either.
 *
 * max_index_bytes: the budget of the index (0: 256 MiB).  A level of heavily
 * overlapping tables needs O(T^2) list entries; when the index would exceed
 * the budget status() is OUT_OF_RANGE, nothing was built, and the caller keeps
 * using LevelMultiGetFilter(cache, tables, ...). */
class LevelIndex {
 public:
  explicit LevelIndex(const vector<TableRange> &tables, uint64_t max_index_bytes = 0);
  ~LevelIndex();
  LevelIndex(const LevelIndex &) = delete;
  LevelIndex &operator=(const LevelIndex &) = delete;
  RC status() const { return status_; }
  size_t tables() const { return tables_.size(); }
  const vector<string_view> &oids() const { return oid_views_; }
  uint32_t longest_list() const; /* no key has more candidates */
  uint32_t mean_list() const;    /* the mean length of a region's list, rounded up */
  /* LevelCandidates from the host copy: no decode, no sort, no sweep -- a
   * binary search and a copy per key */
  void Candidates(const vector<string_view> &user_keys, int64_t seq, vector<uint32_t> &begin,
                  vector<uint32_t> &table) const;
  /* The C-ABI level (adl_bloom_level_create from the same tables and budget),
   * made by the first call: batches that stay on the host never need it.
   * NULL when that failed (device_status()). */
  adl_bloom_level *handle();
  RC device_status() const { return device_status_; }

 private:
  unique_ptr<adl_level::Index> ix_; /* the host copy (level_index_core.hpp) */
  vector<TableRange> tables_;       /* for handle() */
  vector<string_view> oid_views_;
  uint64_t max_index_bytes_;
  std::once_flag handle_once_;
  adl_bloom_level *h_ = nullptr;
  RC device_status_ = OK;
  RC status_;
};

/* LevelMultiGetFilter over a resident index: the same begin / table / maybe /
 * uncached as the call above on the tables the index was built from.  Batches
 * of fewer than ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS keys (0 = never
 * the device) are looked up in the host copy and probed as above; larger ones
 * upload their keys only, and selection, list expansion and the probes all run
 * on the device (adl_bloom_level_multiget). */
RC LevelMultiGetFilter(FilterCache &cache, LevelIndex &level, const vector<string_view> &user_keys, int64_t seq,
                       MultiGetFilterResult &out);

/* The whole revision: its levels in Revision::Get's visiting order
 * (src/revision.cpp:391-403), level 0 first.  The LevelIndex objects are
 * BORROWED and must outlive it; nullptr or a level of no tables is an empty
 * level (skipped, as levels_[i].Empty() is).  Table t of level l has the
 * global id table_base()[l] + t.  status(): BAD_REVISION for more than
 * ADL_BLOOM_MAX_LEVELS (8) levels, a level's own status, OUT_OF_RANGE when the
 * levels' longest lists sum to 2^24 or more. */
class RevisionIndex {
 public:
  explicit RevisionIndex(const vector<LevelIndex *> &levels);
  ~RevisionIndex();
  RevisionIndex(const RevisionIndex &) = delete;
  RevisionIndex &operator=(const RevisionIndex &) = delete;
  RC status() const { return status_; }
  size_t levels() const { return levels_.size(); }
  LevelIndex *level(size_t l) const { return levels_[l]; }
  const vector<uint32_t> &table_base() const { return table_base_; } /* levels() + 1 entries */
  uint32_t longest_list() const { return longest_; }                /* no key has more candidates */
  /* Every level's LevelIndex::Candidates, concatenated per key, level 0
   * first, as global ids (host only) */
  void Candidates(const vector<string_view> &user_keys, int64_t seq, vector<uint32_t> &begin,
                  vector<uint32_t> &table) const;
  /* The C-ABI revision over the levels' handles, made by the first call: NULL
   * when that failed (device_status()). */
  adl_bloom_revision *handle();
  RC device_status() const { return device_status_; }

 private:
  vector<LevelIndex *> levels_;
  vector<uint32_t> table_base_;
  uint32_t longest_ = 0;
  std::once_flag handle_once_;
  adl_bloom_revision *h_ = nullptr;
  RC device_status_ = OK;
  RC status_ = OK;
};

struct RevisionMultiGetResult {
  vector<uint32_t> begin; /* key i's hits: [begin[i], begin[i+1]) */
  vector<uint32_t> table; /* global ids of the tables still to read, in Revision::Get's visiting order */
  vector<uint8_t> level;  /* the level of each hit */
  uint64_t uncached = 0;  /* hits whose table was not in the cache (answered 1) */
};

/* The filter stage of Revision::Get for a batch: per key, the tables of all
 * levels that cover it and whose filter does not rule it out, levels
 * ascending, within a level in Level::Get's order.  The caller reads them in
 * that order and stops at the first that holds the key.  Small batches run
 * LevelMultiGetFilter(cache, LevelIndex&, ...) once per level and keep the
 * pairs answered 1; larger ones are ONE call (adl_bloom_revision_multiget):
 * keys up, hits down.  Both give the same result.  The threshold is
 * ADL_BLOOM_REVISION_DEVICE_MIN_KEYS, or else ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS,
 * where the environment sets one (0 = never the single call); otherwise the
 * measured crossover for the revision's number of non-empty levels: 16 000
 * keys for one, 2 000 for two, 1 000 for three or four, 500 from five on
 * (DESIGN.md §5). */
RC RevisionMultiGetFilter(FilterCache &cache, RevisionIndex &rev, const vector<string_view> &user_keys, int64_t seq,
                          RevisionMultiGetResult &out);

struct RevisionGetResult {
  vector<uint32_t> table;  /* global ids of the tables still to read, in Revision::Get's visiting order */
  vector<uint8_t> level;   /* the level of each */
  uint32_t candidates = 0; /* the tables that cover the key, over all levels */
  uint32_t uncached = 0;   /* hits whose table was not in the cache (answered 1) */
};

/* The filter stage of Revision::Get for ONE key -- DB::Get: the list
 * RevisionMultiGetFilter gives for that key.  The candidates are selected in
 * the levels' host indices, only their oids are resolved in the cache, and all
 * of them are asked about in one request to the cache's resident probe server
 * (adl_bloom_revision_get): no launch for up to ADL_BLOOM_GET_MAX_TABLES (24)
 * candidates and a key of up to ADL_BLOOM_GET_MAX_KEY_BYTES (96) bytes, one
 * launched fan-out probe beyond.  A caller that keeps `out` across calls
 * allocates nothing per call. */
RC RevisionGetFilter(FilterCache &cache, RevisionIndex &rev, string_view user_key, int64_t seq,
                     RevisionGetResult &out);

/* The hits of a revision multi-get table by table: what a reader that opens
 * each table once works from.  Level::Get reads every candidate table of a
 * level and keeps the smallest inner key (src/revision.cpp:279-308), so within
 * a level each group is read whole; the levels are walked ascending
 * (src/revision.cpp:391-403) and a key an earlier level has found is skipped
 * in the later ones. */
struct RevisionReadPlan {
  vector<uint32_t> group_table; /* global ids of the tables with a hit, ascending */
  vector<uint8_t> group_level;  /* the level of each, from table_base */
  vector<uint32_t> group_begin; /* groups + 1 */
  vector<uint32_t> key;         /* indices into user_keys; group g's are key[group_begin[g] .. group_begin[g+1]), ascending */
  vector<uint32_t> level_begin; /* levels + 1: level l's groups are [level_begin[l], level_begin[l+1]) */
  uint64_t uncached = 0;        /* entries whose table was not in the cache (answered 1) */
};

/* The plan of a key-major result (host only): a stable counting sort of the
 * hits on the table id.  table_base: RevisionIndex::table_base(). */
void GroupHitsByTable(const RevisionMultiGetResult &hits, const vector<uint32_t> &table_base, RevisionReadPlan &out);

/* RevisionMultiGetFilter whose result comes back as a plan.  Small batches run
 * it and then GroupHitsByTable; larger ones are ONE call
 * (adl_bloom_revision_read_plan: keys up, the grouping on the device, the plan
 * down).  Both give the same plan.  The threshold is RevisionMultiGetFilter's
 * where the environment sets it (the same knobs; 0 = never the single call);
 * otherwise that function's default or the measured floor, whichever is
 * larger: 3 000 keys for revisions of up to 256 tables, 65 536 beyond
 * ("Read plan"). */
RC RevisionReadPlanFilter(FilterCache &cache, RevisionIndex &rev, const vector<string_view> &user_keys, int64_t seq,
                          RevisionReadPlan &out);

}  // namespace adl
