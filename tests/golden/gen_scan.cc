// Writes the scan_*.sst fixtures and scan_cases.json: for each case the sorted
// runs (scan_<case>_in<r>.sst) by the reference's TableBuilder, and for
// several snapshots what the reference's own DBIter (db/db_iter.cc) over
// NewMergingIterator over Table::Open + NewIterator of those tables does:
// the full forward walk, the full SeekToLast / Prev walk, Seek(k) followed by
// one Prev, and the loop
//   for (it->Seek(start); it->Valid() && n < max && it->key() < limit; it->Next()) ++n;
// for a list of (start, limit, max), each with status().ok() at its end. The
// expectation tests/scan_model.py is pinned against, and
// lvkv_sst_scan_entries_device through it. TEST INFRASTRUCTURE; not part of
// the build. From the repository root, with the reference tree at $REF:
//
//   g++ -O2 -std=c++17 -DLEVELDB_PLATFORM_POSIX=1 -DLEVELDB_HAS_PORT_CONFIG_H=0 \
//       -DHAVE_SNAPPY=0 -DHAVE_ZSTD=0 -I$REF -I$REF/include -w -o /tmp/gen_scan \
//       tests/golden/gen_scan.cc \
//       $(ls $REF/util/*.cc $REF/table/*.cc $REF/db/*.cc | \
//         grep -v -e _test -e testutil -e env_windows -e leveldbutil -e /c.cc) -lpthread
//   /tmp/gen_scan tests/golden
//
// DBIter is given no DBImpl: it touches db_ only in RecordReadSample, once its
// sampling period has run out, so the seed is picked (with the reference's
// Random) such that the first period exceeds four times the case's bytes, and
// every walk gets an iterator of its own. An entry is named by (run, index in
// the run), found through its value: values are unique over a case. A
// position of a walk is given as an index into the forward walk, -1 for an
// iterator that is not Valid(); the generator stops where the reference
// yields an entry the forward walk does not have, or a loop's entries are not
// consecutive in it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "db/db_iter.h"
#include "db/dbformat.h"
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/iterator.h"
#include "leveldb/options.h"
#include "leveldb/table.h"
#include "leveldb/table_builder.h"
#include "table/merger.h"
#include "util/random.h"

namespace {

using leveldb::Slice;
using leveldb::Status;

typedef std::pair<std::string, std::string> Entry;
typedef std::vector<Entry> Run;

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

struct Query {
  int start, limit, max;  // indices into the case's keys; limit -1: none; max -1: none
};

struct Case {
  std::string name;
  std::vector<Run> runs;
  std::vector<uint64_t> snapshots;
  std::vector<std::string> qkeys;  // user keys: seek targets, starts and limits
};

constexpr int kBlockSize = 256;
const uint64_t kMax = leveldb::kMaxSequenceNumber;

std::string dir, json;
const leveldb::InternalKeyComparator* icmp;

void Die(const std::string& what) {
  fprintf(stderr, "gen_scan: %s\n", what.c_str());
  exit(1);
}

leveldb::Options TableOptions() {
  leveldb::Options o;
  o.compression = leveldb::kNoCompression;
  o.block_size = kBlockSize;
  o.comparator = icmp;
  return o;
}

std::string WriteTable(const Run& entries, std::string* blocks) {
  Sink sink;
  leveldb::TableBuilder b(TableOptions(), &sink);
  for (const auto& e : entries) b.Add(e.first, e.second);
  b.Flush();
  const size_t data_appends = sink.appends.size();
  if (!b.Finish().ok()) Die("Finish");
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
  if (f == nullptr) Die("cannot write " + file);
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

// The opened tables of a case, and DBIters over them.
struct Opened {
  std::vector<std::string> images;
  std::vector<std::unique_ptr<Source>> files;
  std::vector<std::unique_ptr<leveldb::Table>> tables;
  std::map<std::string, std::pair<int, int>> by_value;
  uint32_t seed = 0;
  uint64_t period = 0, total_bytes = 0;

  std::unique_ptr<leveldb::Iterator> Iter(uint64_t snapshot) const {
    std::vector<leveldb::Iterator*> children;
    for (const auto& t : tables) children.push_back(t->NewIterator(leveldb::ReadOptions()));
    leveldb::Iterator* merged =
        leveldb::NewMergingIterator(icmp, children.data(), static_cast<int>(children.size()));
    return std::unique_ptr<leveldb::Iterator>(
        leveldb::NewDBIterator(nullptr, leveldb::BytewiseComparator(), merged, snapshot, seed));
  }
  std::pair<int, int> Which(const leveldb::Iterator& it) const {
    const auto at = by_value.find(it.value().ToString());
    if (at == by_value.end()) Die("a value no entry has");
    return at->second;
  }
};

int IndexIn(const std::vector<std::pair<int, int>>& walk, const std::pair<int, int>& e) {
  const auto at = std::find(walk.begin(), walk.end(), e);
  if (at == walk.end()) Die("an entry the forward walk does not have");
  return static_cast<int>(at - walk.begin());
}

std::string Pairs(const std::vector<std::pair<int, int>>& walk) {
  std::string s;
  for (const auto& e : walk)
    s += (s.empty() ? "" : ", ") + std::to_string(e.first) + ", " + std::to_string(e.second);
  return s;
}

const char* Bool(bool b) { return b ? "true" : "false"; }

void Emit(Case c) {
  fprintf(stderr, "%s\n", c.name.c_str());
  const size_t nruns = c.runs.size();
  Opened o;
  std::string inputs, blocks;
  for (size_t r = 0; r < nruns; ++r) {
    Run& run = c.runs[r];
    std::sort(run.begin(), run.end(),
              [](const Entry& a, const Entry& b) { return icmp->Compare(a.first, b.first) < 0; });
    for (size_t j = 0; j < run.size(); ++j) {
      if (!o.by_value.insert({run[j].second, {static_cast<int>(r), static_cast<int>(j)}}).second)
        Die("a value twice");
      o.total_bytes += run[j].first.size() + run[j].second.size();
    }
    o.images.push_back(WriteTable(run, &blocks));
    char file[128];
    snprintf(file, sizeof file, "scan_%s_in%zu.sst", c.name.c_str(), r);
    Save(file, o.images.back());
    inputs += std::string(r ? ",\n      " : "") + "{\"file\": \"" + file + "\", \"entries\": " +
              std::to_string(run.size()) + ", \"blocks\": [" + blocks + "]}";
  }
  const leveldb::Options topt = TableOptions();
  for (size_t r = 0; r < nruns; ++r) {
    o.files.emplace_back(new Source(o.images[r]));
    leveldb::Table* t = nullptr;
    if (!leveldb::Table::Open(topt, o.files.back().get(), o.images[r].size(), &t).ok())
      Die("Table::Open");
    o.tables.emplace_back(t);
  }
  // DBIter's first sampling period (RandomCompactionPeriod, db/db_iter.cc:117-119)
  // has to outlast every walk: none passes an entry more than four times
  for (uint32_t seed = 1;; ++seed) {
    leveldb::Random rnd(seed);
    const uint64_t period = rnd.Uniform(2 * leveldb::config::kReadBytesPeriod);
    if (period > 4 * o.total_bytes + 1024) {
      o.seed = seed;
      o.period = period;
      break;
    }
    if (seed > 1000) Die("no seed");
  }
  if (!(o.period > 4 * o.total_bytes)) Die("the sampling period is too short");

  std::string snaps;
  for (size_t k = 0; k < c.snapshots.size(); ++k) {
    const uint64_t snapshot = c.snapshots[k];
    std::vector<std::pair<int, int>> forward, reverse;
    auto it = o.Iter(snapshot);
    for (it->SeekToFirst(); it->Valid(); it->Next()) forward.push_back(o.Which(*it));
    const bool forward_ok = it->status().ok();
    it = o.Iter(snapshot);
    for (it->SeekToLast(); it->Valid(); it->Prev()) reverse.push_back(o.Which(*it));
    const bool reverse_ok = it->status().ok();

    std::string seeks;
    for (size_t q = 0; q < c.qkeys.size(); ++q) {
      it = o.Iter(snapshot);
      it->Seek(c.qkeys[q]);
      const int at = it->Valid() ? IndexIn(forward, o.Which(*it)) : -1;
      const bool seek_ok = it->status().ok();
      int prev = -2;  // (Prev asserts Valid())
      bool prev_ok = seek_ok;
      if (it->Valid()) {
        it->Prev();
        prev = it->Valid() ? IndexIn(forward, o.Which(*it)) : -1;
        prev_ok = it->status().ok();
      }
      seeks += std::string(q ? ", " : "") + "[" + std::to_string(q) + ", " + std::to_string(at) +
               ", " + Bool(seek_ok) + ", " + std::to_string(prev) + ", " + Bool(prev_ok) + "]";
    }

    // every start with every limit (and none); max: none, then 0, 1, the
    // exact count and two more than it, in turn
    std::string queries;
    int turn = 0;
    const int nk = static_cast<int>(c.qkeys.size());
    for (int s = 0; s < nk; ++s) {
      for (int l = -1; l < nk; ++l) {
        int exact = 0;
        for (int pass = 0; pass < 2; ++pass) {
          int max = -1;
          if (pass == 1) {
            const int pick = turn++ % 4;
            max = pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? exact : exact + 2;
          }
          it = o.Iter(snapshot);
          int n = 0, first = -1;
          for (it->Seek(c.qkeys[s]);
               it->Valid() && (max < 0 || n < max) &&
               (l < 0 || it->key().compare(Slice(c.qkeys[l])) < 0);
               it->Next()) {
            const int at = IndexIn(forward, o.Which(*it));
            if (n == 0) first = at;
            else if (at != first + n) Die("a loop's entries are not consecutive");
            ++n;
          }
          if (n == 0 && it->Valid()) first = IndexIn(forward, o.Which(*it));
          if (pass == 0) exact = n;
          queries += std::string(queries.empty() ? "" : ", ") + "[" + std::to_string(s) + ", " +
                     std::to_string(l) + ", " + std::to_string(max) + ", " + std::to_string(first) +
                     ", " + std::to_string(n) + ", " + Bool(it->status().ok()) + "]";
        }
      }
    }
    snaps += std::string(k ? ",\n      " : "") + "{\"snapshot\": " + std::to_string(snapshot) +
             ", \"forward\": [" + Pairs(forward) + "], \"forward_ok\": " + Bool(forward_ok) +
             ",\n       \"reverse\": [" + Pairs(reverse) + "], \"reverse_ok\": " + Bool(reverse_ok) +
             ",\n       \"seek_prev\": [" + seeks + "],\n       \"queries\": [" + queries + "]}";
  }
  std::string keys;
  for (const std::string& q : c.qkeys) keys += (keys.empty() ? "\"" : ", \"") + Hex(q) + "\"";
  json += std::string(json.empty() ? "" : ",\n") + "  \"" + c.name + "\": {\"block_size\": " +
          std::to_string(kBlockSize) + ", \"seed\": " + std::to_string(o.seed) +
          ", \"first_period\": " + std::to_string(o.period) + ", \"total_bytes\": " +
          std::to_string(o.total_bytes) + ",\n    \"inputs\": [" + inputs + "],\n    \"qkeys\": [" +
          keys + "],\n    \"snapshots\": [" + snaps + "]}";
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

// (a deletion gets a value too, so that a walk that yielded one would be told)
Entry E(const std::string& user, uint64_t seq, int type = 1) { return {IKey(user, seq, type), Val()}; }

}  // namespace

int main(int argc, char** argv) {
  dir = argc > 1 ? argv[1] : ".";
  icmp = new leveldb::InternalKeyComparator(leveldb::BytewiseComparator());

  {  // one user key in five versions across three runs, between plain neighbours;
     // snapshots above, between and below the versions
    Case c{"five_versions", {{}, {}, {}}, {kMax, 600, 500, 450, 400, 350, 250, 150, 100, 99, 0},
           {"", "a", "b", "five", "five\x01", "g", "h", "z"}};
    c.runs[0].push_back(E("b", 120));
    c.runs[1].push_back(E("five", 500));
    c.runs[0].push_back(E("five", 400));
    c.runs[2].push_back(E("five", 300));
    c.runs[0].push_back(E("five", 200));
    c.runs[2].push_back(E("five", 100));
    c.runs[1].push_back(E("g", 110));
    c.runs[2].push_back(E("h", 700));  // above most snapshots: a key with no version to see
    Emit(c);
  }
  {  // a deletion as the newest, a middle and the oldest eligible version; a
     // deletion above the snapshot over a value below it
    Case c{"deletions", {{}, {}},
           {kMax, 100, 90, 80, 70, 60, 50, 0},
           {"", "d-mid", "d-new", "d-newz", "d-old", "e-above", "f", "zz"}};
    c.runs[0].push_back(E("c", 10));
    c.runs[0].push_back(E("d-new", 90, 0));
    c.runs[1].push_back(E("d-new", 80));
    c.runs[0].push_back(E("d-new", 70));
    c.runs[1].push_back(E("d-mid", 90));
    c.runs[0].push_back(E("d-mid", 80, 0));
    c.runs[1].push_back(E("d-mid", 70));
    c.runs[0].push_back(E("d-old", 90));
    c.runs[1].push_back(E("d-old", 80));
    c.runs[0].push_back(E("d-old", 70, 0));
    c.runs[1].push_back(E("e-above", 100, 0));
    c.runs[0].push_back(E("e-above", 60));
    c.runs[1].push_back(E("f", 20));
    c.runs[1].push_back(E("g-alone", 30, 0));  // a deletion on its own, the last key
    Emit(c);
  }
  {  // keys that do not parse (type byte 2): between two versions of one user
     // key, before the first visible entry, after the last
    Case c{"unparsable", {{}, {}, {}},
           {kMax, 95, 85, 75, 65, 0},
           {"", "a", "b", "err", "err\x01", "m", "n", "zz", "zzz"}};
    c.runs[0].push_back(E("a", 50, 2));   // before everything that can be seen
    c.runs[1].push_back(E("b", 60));
    c.runs[0].push_back(E("err", 90));
    c.runs[1].push_back(E("err", 80, 2));
    c.runs[2].push_back(E("err", 70));
    c.runs[0].push_back(E("err", 60));
    c.runs[1].push_back(E("m", 40));
    c.runs[2].push_back(E("n", 41));
    c.runs[2].push_back(E("zz", 30, 2));  // after the last
    Emit(c);
  }
  {  // an unparsable key in the middle only: walks before it stay clean
    Case c{"unparsable_middle", {{}, {}},
           {kMax, 10},
           {"", "a", "b", "c", "d", "e", "f"}};
    c.runs[0].push_back(E("a", 5));
    c.runs[1].push_back(E("b", 6));
    c.runs[0].push_back(E("c", 7, 2));
    c.runs[0].push_back(E("c", 4, 0xff));
    c.runs[1].push_back(E("d", 8));
    c.runs[0].push_back(E("e", 9));
    Emit(c);
  }
  {  // the same internal key in three runs
    Case c{"equal_keys", {{}, {}, {}, {}}, {kMax, 77, 76, 0}, {"", "k0003", "same", "same0", "t"}};
    for (int i = 0; i < 8; ++i) {
      char key[16];
      snprintf(key, sizeof key, "k%04d", i);
      c.runs[i % 4].push_back(E(key, 200 + i));
      c.runs[(i + 1) % 4].push_back(E(key, 20 + i));
    }
    for (int r : {3, 1, 2}) c.runs[r].push_back(E("same", 77));
    for (int r : {0, 3}) c.runs[r].push_back(E("same", 60, 0));
    c.runs[0].push_back(E("t", 5));
    c.runs[1].push_back(E("t", 5));
    Emit(c);
  }
  {  // user keys that are prefixes of one another, the empty user key, sequence
     // 0 and kMaxSequenceNumber
    Case c{"prefixes", {{}, {}},
           {kMax, kMax - 1, 31, 30, 1, 0},
           {"", std::string("\0", 1), "pr", "pre", "pref", "prefi", "prefix", "prefiy", "\xff", "\xff\xff"}};
    c.runs[0].push_back(E("", 9));
    c.runs[1].push_back(E("", 4, 0));
    c.runs[1].push_back(E("", 0));
    c.runs[0].push_back(E("pre", 30));
    c.runs[1].push_back(E("prefix", 31));
    c.runs[0].push_back(E("pref", 32));
    c.runs[1].push_back(E("pre", 12, 0));
    c.runs[0].push_back(E("pre", 0));
    c.runs[0].push_back(E("\xff", kMax));
    c.runs[1].push_back(E("\xff", kMax - 1));
    c.runs[1].push_back(E("\xff", 0, 0));
    Emit(c);
  }
  {  // an empty run among three
    Case c{"empty_run", {{}, {}, {}}, {kMax, 150, 0}, {"", "k0004", "k0004x", "k0011", "k9"}};
    for (int i = 0; i < 12; ++i) {
      char key[16];
      snprintf(key, sizeof key, "k%04d", i);
      c.runs[i % 2 ? 0 : 2].push_back(E(key, 140 + 2 * i, i % 5 == 3 ? 0 : 1));
      if (i % 3 == 0) c.runs[i % 2 ? 2 : 0].push_back(E(key, 100 + i));
    }
    Emit(c);
  }
  {  // one run only, more than a block of it
    Case c{"one_run", {{}}, {kMax, 130, 0}, {"", "k0000", "k0017", "k0017+", "k0039", "k004"}};
    for (int i = 0; i < 40; ++i) {
      char key[16];
      snprintf(key, sizeof key, "k%04d", i);
      c.runs[0].push_back(E(key, 100 + 3 * i));
      if (i % 5 == 0) c.runs[0].push_back(E(key, 50 + i, i % 10 == 0 ? 0 : 1));
      if (i % 7 == 0) c.runs[0].push_back(E(key, 250 + i, 0));
    }
    Emit(c);
  }
  {  // nothing at all
    Case c{"no_entries", {{}}, {kMax, 0}, {"", "a"}};
    Emit(c);
  }
  FILE* f = fopen((dir + "/scan_cases.json").c_str(), "w");
  if (f == nullptr) Die("cannot write scan_cases.json");
  fprintf(f, "{\n%s\n}\n", json.c_str());
  fclose(f);
  return 0;
}
