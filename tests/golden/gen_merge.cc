// Writes the merge_*.sst fixtures and merge_cases.json: for each case the
// sorted input tables (merge_<case>_in<r>.sst) by the reference's
// TableBuilder, the order in which the reference's own
// NewMergingIterator over Table::Open + NewIterator of those tables hands
// their entries out, as (run, index in the run) pairs, and for each
// (smallest_snapshot, deeper ranges) setting the drop flag of every merged
// entry -- the loop of db/db_impl.cc:1022-1055 restated below with the
// reference's ParseInternalKey and comparators, IsBaseLevelForKey
// (db/version_set.cc:1518-1537) as "in none of the ranges" -- and the table
// the reference's TableBuilder writes from the survivors
// (merge_<case>_s<k>_out.sst). The expectation tests/sst_merge_model.py is
// pinned against, and lvkv_sst_merge_entries_device through it. TEST
// INFRASTRUCTURE; not part of the build. From the repository root, with the
// reference tree at $REF:
//
//   g++ -O2 -std=c++17 -DLEVELDB_PLATFORM_POSIX=1 -DLEVELDB_HAS_PORT_CONFIG_H=0 \
//       -I$REF -I$REF/include -w -o /tmp/gen_merge tests/golden/gen_merge.cc \
//       $REF/util/{crc32c,coding,comparator,options,status,env,env_posix,logging,bloom,hash,filter_policy,cache}.cc \
//       $REF/table/{table,table_builder,block,block_builder,filter_block,format,iterator,merger,two_level_iterator}.cc \
//       $REF/db/dbformat.cc -lpthread
//   /tmp/gen_merge tests/golden
//
// Flags: 0 kept, 1 hidden (rule A), 2 obsolete deletion. The asserts of
// TableBuilder::Add are live (no NDEBUG): a run that is not strictly
// ascending under its comparator stops the generator.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "db/dbformat.h"
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/filter_policy.h"
#include "leveldb/iterator.h"
#include "leveldb/options.h"
#include "leveldb/table.h"
#include "leveldb/table_builder.h"
#include "table/merger.h"

namespace {

using leveldb::Slice;
using leveldb::Status;

typedef std::pair<std::string, std::string> Entry;
typedef std::vector<Entry> Run;

// The file as a string, and where every Append began and how long it was:
// WriteRawBlock appends a block's contents, then its 5-byte trailer.
class Sink : public leveldb::WritableFile {
 public:
  Status Append(const Slice& d) override {
    appends.push_back({data.size(), d.size()});
    data.append(d.data(), d.size());
    return Status::OK();
  }
  Status Close() override { return Status::OK(); }
  Status Flush() override { return Status::OK(); }
  Status Sync() override { return Status::OK(); }
  std::string data;
  std::vector<std::pair<size_t, size_t>> appends;
};

class Source : public leveldb::RandomAccessFile {
 public:
  explicit Source(const std::string& d) : data_(d) {}
  Status Read(uint64_t offset, size_t n, Slice* result, char* scratch) const override {
    if (offset > data_.size()) return Status::InvalidArgument("read past the end");
    if (offset + n > data_.size()) n = data_.size() - offset;
    *result = Slice(data_.data() + offset, n);
    return Status::OK();
  }

 private:
  const std::string& data_;
};

struct Setting {
  uint64_t snapshot;
  std::vector<std::pair<std::string, std::string>> deeper;  // smallest, largest user keys
};

struct Case {
  std::string name;
  int key_format;
  std::vector<Run> runs;
  std::vector<Setting> settings;
};

constexpr int kInBlockSize = 256, kOutBlockSize = 512, kBits = 10;
const uint64_t kMax = leveldb::kMaxSequenceNumber;

std::string dir, json;
const leveldb::FilterPolicy* bloom;
const leveldb::InternalKeyComparator* icmp;
const leveldb::InternalFilterPolicy* ipolicy;

leveldb::Options TableOptions(int key_format, int block_size) {
  leveldb::Options o;
  o.compression = leveldb::kNoCompression;
  o.block_size = block_size;
  o.filter_policy = bloom;
  if (key_format == 1) {
    o.comparator = icmp;
    o.filter_policy = ipolicy;
  }
  return o;
}

// The table of `entries`; *blocks: the data blocks' handles as JSON.
std::string WriteTable(int key_format, int block_size, const Run& entries, std::string* blocks) {
  Sink sink;
  leveldb::TableBuilder b(TableOptions(key_format, block_size), &sink);
  for (const auto& e : entries) b.Add(e.first, e.second);
  b.Flush();
  const size_t data_appends = sink.appends.size();
  if (!b.Finish().ok()) abort();
  blocks->clear();
  char buf[96];
  for (size_t i = 0; i + 1 < data_appends; i += 2) {
    snprintf(buf, sizeof buf, "%s{\"offset\": %zu, \"size\": %zu}", i ? ", " : "",
             sink.appends[i].first, sink.appends[i].second);
    *blocks += buf;
  }
  return sink.data;
}

void Save(const std::string& file, const std::string& data) {
  FILE* f = fopen((dir + "/" + file).c_str(), "wb");
  if (f == nullptr) abort();
  fwrite(data.data(), 1, data.size(), f);
  fclose(f);
}

std::string Hex(const std::string& s) {
  std::string out;
  char buf[4];
  for (unsigned char c : s) {
    snprintf(buf, sizeof buf, "%02x", c);
    out += buf;
  }
  return out;
}

// Compaction::IsBaseLevelForKey for files given in any order.
bool BaseLevel(const Setting& s, const Slice& user_key) {
  const leveldb::Comparator* ucmp = leveldb::BytewiseComparator();
  for (const auto& r : s.deeper)
    if (ucmp->Compare(user_key, r.second) <= 0 && ucmp->Compare(user_key, r.first) >= 0)
      return false;
  return true;
}

// db/db_impl.cc:1022-1055 over the merged keys.
std::string Drops(const Setting& s, const std::vector<std::string>& keys) {
  const leveldb::Comparator* ucmp = leveldb::BytewiseComparator();
  std::string flags;
  leveldb::ParsedInternalKey ikey;
  std::string current_user_key;
  bool has_current_user_key = false;
  leveldb::SequenceNumber last_sequence_for_key = kMax;
  for (const std::string& key : keys) {
    char drop = '0';
    if (!leveldb::ParseInternalKey(key, &ikey)) {
      current_user_key.clear();
      has_current_user_key = false;
      last_sequence_for_key = kMax;
    } else {
      if (!has_current_user_key || ucmp->Compare(ikey.user_key, Slice(current_user_key)) != 0) {
        current_user_key.assign(ikey.user_key.data(), ikey.user_key.size());
        has_current_user_key = true;
        last_sequence_for_key = kMax;
      }
      if (last_sequence_for_key <= s.snapshot) {
        drop = '1';
      } else if (ikey.type == leveldb::kTypeDeletion && ikey.sequence <= s.snapshot &&
                 BaseLevel(s, ikey.user_key)) {
        drop = '2';
      }
      last_sequence_for_key = ikey.sequence;
    }
    flags += drop;
  }
  return flags;
}

void Emit(Case c) {
  const size_t nruns = c.runs.size();
  fprintf(stderr, "%s\n", c.name.c_str());
  const leveldb::Comparator* cmp = TableOptions(c.key_format, kInBlockSize).comparator;
  for (Run& r : c.runs)
    std::sort(r.begin(), r.end(),
              [cmp](const Entry& a, const Entry& b) { return cmp->Compare(a.first, b.first) < 0; });
  std::vector<std::string> images(nruns);
  std::string inputs, blocks;
  for (size_t r = 0; r < nruns; ++r) {
    images[r] = WriteTable(c.key_format, kInBlockSize, c.runs[r], &blocks);
    char file[128];
    snprintf(file, sizeof file, "merge_%s_in%zu.sst", c.name.c_str(), r);
    Save(file, images[r]);
    inputs += std::string(r ? ",\n      " : "") + "{\"file\": \"" + file + "\", \"entries\": " +
              std::to_string(c.runs[r].size()) + ", \"blocks\": [" + blocks + "]}";
  }
  // the reference's walk: Table::Open, NewIterator, NewMergingIterator
  const leveldb::Options o = TableOptions(c.key_format, kInBlockSize);
  std::vector<std::unique_ptr<Source>> files;
  std::vector<std::unique_ptr<leveldb::Table>> tables;
  std::vector<leveldb::Iterator*> children;
  for (size_t r = 0; r < nruns; ++r) {
    files.emplace_back(new Source(images[r]));
    leveldb::Table* t = nullptr;
    if (!leveldb::Table::Open(o, files.back().get(), images[r].size(), &t).ok()) abort();
    tables.emplace_back(t);
    children.push_back(t->NewIterator(leveldb::ReadOptions()));
  }
  std::unique_ptr<leveldb::Iterator> it(
      leveldb::NewMergingIterator(o.comparator, children.data(), static_cast<int>(nruns)));
  // (run, index) of each entry handed out: the value says which entry it is
  std::vector<size_t> next(nruns, 0);
  std::vector<std::string> keys;
  Run merged;
  std::string order;
  for (it->SeekToFirst(); it->Valid(); it->Next()) {
    // the entry's run: the one whose next entry has this key and this very
    // value (values are unique over a case)
    size_t run = nruns;
    for (size_t r = 0; r < nruns && run == nruns; ++r)
      if (next[r] < c.runs[r].size() && it->key() == Slice(c.runs[r][next[r]].first) &&
          it->value() == Slice(c.runs[r][next[r]].second))
        run = r;
    if (run == nruns) abort();
    order += (order.empty() ? "" : ", ") + std::to_string(run) + ", " + std::to_string(next[run]);
    ++next[run];
    keys.push_back(it->key().ToString());
    merged.push_back({it->key().ToString(), it->value().ToString()});
  }
  if (!it->status().ok()) abort();
  for (size_t r = 0; r < nruns; ++r)
    if (next[r] != c.runs[r].size()) abort();

  std::string settings;
  for (size_t k = 0; k < c.settings.size(); ++k) {
    const Setting& s = c.settings[k];
    const std::string flags = Drops(s, keys);
    Run kept;
    for (size_t i = 0; i < merged.size(); ++i)
      if (flags[i] == '0') kept.push_back(merged[i]);
    char file[128];
    snprintf(file, sizeof file, "merge_%s_s%zu_out.sst", c.name.c_str(), k);
    Save(file, WriteTable(c.key_format, kOutBlockSize, kept, &blocks));
    std::string deeper;
    for (const auto& r : s.deeper)
      deeper += std::string(deeper.empty() ? "" : ", ") + "[\"" + Hex(r.first) + "\", \"" +
                Hex(r.second) + "\"]";
    settings += std::string(k ? ",\n      " : "") + "{\"smallest_snapshot\": " +
                std::to_string(s.snapshot) + ", \"deeper\": [" + deeper + "], \"drops\": \"" +
                flags + "\", \"out\": \"" + file + "\"}";
  }
  json += std::string(json.empty() ? "" : ",\n") + "  \"" + c.name + "\": {\"key_format\": " +
          std::to_string(c.key_format) + ", \"in_block_size\": " + std::to_string(kInBlockSize) +
          ", \"out_block_size\": " + std::to_string(kOutBlockSize) + ", \"bits_per_key\": " +
          std::to_string(kBits) + ",\n    \"inputs\": [" + inputs + "],\n    \"order\": [" + order +
          "],\n    \"settings\": [" + settings + "]}";
}

int serial = 0;
// A value no other entry of the generator has.
std::string Val() {
  char buf[32];
  snprintf(buf, sizeof buf, "v%05d", serial++);
  return std::string(buf) + std::string(serial % 7, '.');
}

std::string IKey(const std::string& user, uint64_t seq, int type = 1) {
  std::string k = user;
  const uint64_t packed = (seq << 8) | static_cast<uint64_t>(type);
  for (int i = 0; i < 8; ++i) k.push_back(static_cast<char>(packed >> (8 * i)));
  return k;
}

Entry E(const std::string& user, uint64_t seq, int type = 1) {
  return {IKey(user, seq, type), type == 0 ? std::string() + Val().substr(0, 6) : Val()};
}

std::string Num(const char* fmt, int i) {
  char buf[32];
  snprintf(buf, sizeof buf, fmt, i);
  return buf;
}

const std::vector<Setting> kPlain = {{0, {}}, {kMax, {}}, {150, {{"k0010", "k0020"}}}};

}  // namespace

int main(int argc, char** argv) {
  dir = argc > 1 ? argv[1] : ".";
  bloom = leveldb::NewBloomFilterPolicy(kBits);
  icmp = new leveldb::InternalKeyComparator(leveldb::BytewiseComparator());
  ipolicy = new leveldb::InternalFilterPolicy(bloom);

  {  // one run: the merge is the identity, the drops are not
    Case c{"one_run", 1, {{}}, kPlain};
    for (int i = 0; i < 40; ++i) {
      c.runs[0].push_back(E(Num("k%04d", i), 100 + 3 * i));
      if (i % 5 == 0) c.runs[0].push_back(E(Num("k%04d", i), 50 + i, i % 10 == 0 ? 0 : 1));
    }
    Emit(c);
  }
  {  // strict interleave
    Case c{"two_interleaved", 1, {{}, {}}, kPlain};
    for (int i = 0; i < 60; ++i) c.runs[i % 2].push_back(E(Num("k%04d", i), 120 + i, i % 9 ? 1 : 0));
    Emit(c);
  }
  {  // all of run 0 before all of run 1
    Case c{"two_in_order", 1, {{}, {}}, kPlain};
    for (int i = 0; i < 40; ++i) c.runs[i / 20].push_back(E(Num("k%04d", i), 140 + i));
    Emit(c);
  }
  {  // all of run 1 before all of run 0
    Case c{"two_reversed", 1, {{}, {}}, kPlain};
    for (int i = 0; i < 40; ++i) c.runs[1 - i / 20].push_back(E(Num("k%04d", i), 140 + i));
    Emit(c);
  }
  for (int empty = 0; empty < 3; ++empty) {  // an empty first, middle and last run
    const char* names[] = {"three_empty_first", "three_empty_middle", "three_empty_last"};
    Case c{names[empty], 1, {{}, {}, {}}, kPlain};
    const int a = empty == 0 ? 1 : 0, b = empty == 2 ? 1 : 2;
    for (int i = 0; i < 30; ++i) {
      c.runs[i % 3 == 0 ? a : b].push_back(E(Num("k%04d", i), 160 - i));
      if (i % 4 == 0) c.runs[i % 3 == 0 ? b : a].push_back(E(Num("k%04d", i), 20 + i, 0));
    }
    Emit(c);
  }
  {  // a one-entry run inside a long one
    Case c{"one_in_long", 1, {{}, {}}, kPlain};
    for (int i = 0; i < 50; ++i) c.runs[0].push_back(E(Num("k%04d", 2 * i), 100 + i));
    c.runs[1].push_back(E("k0031", 7));
    Emit(c);
  }
  {  // five runs: what the comparator and the drop rule have to tell apart
    Case c{"five_runs", 1, {{}, {}, {}, {}, {}},
           {{0, {}}, {kMax, {}}, {250, {}}, {5, {{"a", "b"}}}, {299, {{"zzz", "zzzz"}}}}};
    // an 8-byte internal key: the empty user key, in two versions
    c.runs[0].push_back(E("", 9));
    c.runs[3].push_back(E("", 4, 0));
    // one user key in five versions across three runs
    c.runs[0].push_back(E("five", 500));
    c.runs[2].push_back(E("five", 400, 0));
    c.runs[0].push_back(E("five", 300));
    c.runs[4].push_back(E("five", 200));
    c.runs[2].push_back(E("five", 100));
    // sequences 5 and 300: the trailer's bytes order them the other way
    c.runs[1].push_back(E("seq", 300));
    c.runs[3].push_back(E("seq", 5));
    // a user key that is a prefix of another
    c.runs[4].push_back(E("pre", 30));
    c.runs[1].push_back(E("prefix", 31));
    c.runs[2].push_back(E("pref", 32));
    c.runs[0].push_back(E("pre", 12, 0));
    // an error key, type byte 2, between two versions of one user key
    c.runs[1].push_back(E("err", 90));
    c.runs[2].push_back(E("err", 80, 2));
    c.runs[3].push_back(E("err", 70));
    c.runs[4].push_back(E("err", 60));
    Emit(c);
  }
  {  // the same internal key in three runs: all come out, the lowest run's
     // first (a table of the survivors only where the later ones are hidden)
    Case c{"equal_keys", 1, {{}, {}, {}, {}}, {{kMax, {}}, {77, {}}}};
    for (int i = 0; i < 12; ++i) c.runs[i % 4].push_back(E(Num("k%04d", i), 200 + i));
    for (int r : {3, 1, 2}) c.runs[r].push_back(E("same", 77));
    for (int r : {0, 3}) c.runs[r].push_back(E("k0005", 70, 0));
    Emit(c);
  }
  {  // deletions against the snapshot and the deeper levels' ranges
    const std::vector<std::pair<std::string, std::string>> ranges = {{"d30", "d40"}, {"d10", "d20"}, {"d15", "d18"}};
    Case c{"deletions", 1, {{}, {}},
           {{100, ranges}, {99, ranges}, {100, {}}, {kMax, ranges}, {0, ranges}}};
    // at the snapshot (100) and below it (60): inside a range, on its
    // smallest, on its largest, just outside both ends
    const char* users[] = {"d0z", "d1", "d10", "d15", "d20", "d200", "d21", "d30", "d35", "d40", "d400"};
    int i = 0;
    for (const char* u : users) {
      c.runs[i % 2].push_back(E(u, 100, 0));
      c.runs[1 - i % 2].push_back(E(u, 60 - i));
      ++i;
    }
    for (const char* u : users) {
      const std::string below = std::string("e") + u;
      c.runs[i % 2].push_back(E(below, 60, 0));
      c.runs[1 - i % 2].push_back(E(below, 50));
      ++i;
    }
    // above the snapshot
    c.runs[0].push_back(E("f-above", 101, 0));
    c.runs[1].push_back(E("f-above", 40));
    // a deletion that is also hidden: it counts as hidden
    c.runs[1].push_back(E("g-hidden", 90));
    c.runs[0].push_back(E("g-hidden", 80, 0));
    c.runs[1].push_back(E("g-hidden", 70));
    // a deletion on its own
    c.runs[0].push_back(E("h-alone", 10, 0));
    Emit(c);
  }
  {  // sequence 0
    Case c{"sequence_zero", 1, {{}, {}, {}}, {{0, {}}, {1, {}}, {kMax, {{"z1", "z1"}}}}};
    c.runs[0].push_back(E("z0", 3));
    c.runs[1].push_back(E("z0", 0));
    c.runs[2].push_back(E("z0", 0, 0));
    c.runs[1].push_back(E("z1", 0, 0));
    c.runs[0].push_back(E("z2", 0, 0));
    c.runs[2].push_back(E("z3", 0));
    c.runs[0].push_back(E("z4", kMax));
    c.runs[1].push_back(E("z4", kMax, 0));
    c.runs[2].push_back(E("z4", kMax - 1));
    Emit(c);
  }
  {  // byte-wise keys, equal ones in both runs
    Case c{"bytes_two", 0, {{}, {}}, {}};
    for (int i = 0; i < 40; ++i) {
      if (i % 3 != 1) c.runs[0].push_back({Num("b%03d", i), Val()});
      if (i % 3 != 2) c.runs[1].push_back({Num("b%03d", i), Val()});
    }
    Emit(c);
  }
  {  // byte-wise keys: prefixes, high bytes, an empty run, a short one
    Case c{"bytes_three", 0, {{}, {}, {}, {}}, {}};
    c.runs[0] = {{"", Val()}, {"a", Val()}, {"ab", Val()}, {std::string("ab\0", 3), Val()},
                 {"b", Val()}, {"\xff", Val()}, {"\xff\xff", Val()}};
    c.runs[2] = {{"a", Val()}, {"aa", Val()}, {"abc", Val()}, {"\x7f", Val()}, {"\x80", Val()},
                 {"\xff", Val()}};
    c.runs[3] = {{"ab", Val()}};
    Emit(c);
  }
  FILE* f = fopen((dir + "/merge_cases.json").c_str(), "w");
  fprintf(f, "{\n%s\n}\n", json.c_str());
  fclose(f);
  return 0;
}
