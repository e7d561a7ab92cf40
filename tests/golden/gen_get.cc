// Writes the get_*.sst fixtures and get_cases.json: tables by the reference's
// TableBuilder (internal keys with and without the bloom policy, byte-wise
// keys, no compression and Snappy, block_restart_interval 1, 2 and 16, one
// entry, one block, many blocks), and for every query key of a table what the
// reference's own Table::InternalGet did with it, reached as TableCache::Get
// reaches it: whether the callback ran, the entry it was handed, the Status,
// and whether a data block was read at all (a key the filter turned away
// reads none; absent keys the filter lets through are found by search and
// recorded as such). Beside it, for every query, where Block::Iter::Seek
// lands on the index block and on every data block directly -- valid or not,
// the key, the status -- which pins the seek apart from the filter. The
// expectation tests/sst_get_model.py is pinned against, and
// lvkv_sst_get_locate_device / lvkv_sst_get_seek_device through it. TEST
// INFRASTRUCTURE; not part of the build. From the repository root, with the
// reference tree at $REF and libsnappy 1.1.8 under $SNAPPY:
//
//   g++ -O2 -std=c++17 -static-libstdc++ -DLEVELDB_PLATFORM_POSIX=1 \
//       -DLEVELDB_HAS_PORT_CONFIG_H=0 -DHAVE_SNAPPY=1 \
//       -I$REF -I$REF/include -I$SNAPPY/include -w -o /tmp/gen_get tests/golden/gen_get.cc \
//       $REF/util/{crc32c,coding,comparator,options,status,env,env_posix,logging,bloom,hash,filter_policy,cache}.cc \
//       $REF/table/{table,table_builder,block,block_builder,filter_block,format,iterator,two_level_iterator}.cc \
//       $REF/db/dbformat.cc $SNAPPY/lib/libsnappy.so.1.1.8 -Wl,-rpath,$SNAPPY/lib -lpthread
//   /tmp/gen_get tests/golden
//
// A seek is written "V:<key in hex>" where it is valid, "E" where it is not
// and the status is OK, "C:<status>" otherwise.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
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
#include "table/block.h"
#include "table/format.h"

namespace leveldb {
// Table::InternalGet is TableCache's to call (include/leveldb/table.h:62).
class TableCache {
 public:
  static Status Get(Table* t, const Slice& k, void* arg,
                    void (*handle_result)(void*, const Slice&, const Slice&)) {
    return t->InternalGet(ReadOptions(), k, arg, handle_result);
  }
};
}  // namespace leveldb

namespace {

using leveldb::Slice;
using leveldb::Status;

typedef std::pair<std::string, std::string> Entry;

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
    ++reads;
    if (offset > data_.size()) return Status::InvalidArgument("read past the end");
    if (offset + n > data_.size()) n = data_.size() - offset;
    *result = Slice(data_.data() + offset, n);
    return Status::OK();
  }
  mutable int reads = 0;

 private:
  const std::string& data_;
};

struct TableCase {
  std::string name;
  int key_format;
  bool filter;
  bool snappy;
  int restart_interval;
  int block_size;
  std::vector<Entry> entries;
};

std::string dir, json;
const leveldb::FilterPolicy* bloom;
const leveldb::InternalKeyComparator* icmp;
const leveldb::InternalFilterPolicy* ipolicy;

std::string Hex(const Slice& s) {
  std::string out;
  char buf[4];
  for (size_t i = 0; i < s.size(); ++i) {
    snprintf(buf, sizeof buf, "%02x", static_cast<unsigned char>(s[i]));
    out += buf;
  }
  return out;
}

std::string IKey(const std::string& user, uint64_t seq, int type = 1) {
  std::string k = user;
  const uint64_t packed = (seq << 8) | static_cast<uint64_t>(type);
  for (int i = 0; i < 8; ++i) k.push_back(static_cast<char>(packed >> (8 * i)));
  return k;
}

std::string Num(const char* fmt, int i, int j = 0) {
  char buf[48];
  snprintf(buf, sizeof buf, fmt, i, j);
  return buf;
}

int serial = 0;
std::string Val() {
  char buf[32];
  snprintf(buf, sizeof buf, "v%04d", serial++);
  return std::string(buf) + std::string(serial % 5, '.');
}

std::string SeekString(leveldb::Iterator* it) {
  if (it->Valid()) return "V:" + Hex(it->key());
  return it->status().ok() ? "E" : "C:" + it->status().ToString();
}

struct Saved {
  bool called = false;
  std::string key, value;
};

void Save(void* arg, const Slice& k, const Slice& v) {
  Saved* s = reinterpret_cast<Saved*>(arg);
  s->called = true;
  s->key = k.ToString();
  s->value = v.ToString();
}

leveldb::Block* ReadOne(const Source& file, uint64_t off, uint64_t size) {
  leveldb::BlockHandle h;
  h.set_offset(off);
  h.set_size(size);
  leveldb::BlockContents c;
  leveldb::ReadOptions ro;
  ro.verify_checksums = true;
  if (!leveldb::ReadBlock(const_cast<Source*>(&file), ro, h, &c).ok()) abort();
  return new leveldb::Block(c);
}

void Emit(TableCase c, const std::vector<std::string>& fixed_queries, bool search_false_positives) {
  fprintf(stderr, "%s\n", c.name.c_str());
  leveldb::Options o;
  o.compression = c.snappy ? leveldb::kSnappyCompression : leveldb::kNoCompression;
  o.block_size = c.block_size;
  o.block_restart_interval = c.restart_interval;
  o.filter_policy = c.filter ? bloom : nullptr;
  if (c.key_format == 1) {
    o.comparator = icmp;
    o.filter_policy = c.filter ? ipolicy : nullptr;
  }
  const leveldb::Comparator* cmp = o.comparator;
  std::sort(c.entries.begin(), c.entries.end(),
            [cmp](const Entry& a, const Entry& b) { return cmp->Compare(a.first, b.first) < 0; });
  Sink sink;
  leveldb::TableBuilder b(o, &sink);
  for (const auto& e : c.entries) b.Add(e.first, e.second);
  b.Flush();
  const size_t data_appends = sink.appends.size();
  if (!b.Finish().ok()) abort();
  const std::string file = "get_" + c.name + ".sst";
  {
    FILE* f = fopen((dir + "/" + file).c_str(), "wb");
    if (f == nullptr) abort();
    fwrite(sink.data.data(), 1, sink.data.size(), f);
    fclose(f);
  }
  // blocks in the order written: data, [filter], metaindex, index, footer
  const size_t fa = data_appends, ia = data_appends + (c.filter ? 4 : 2);
  char buf[128];
  std::string blocks;
  for (size_t i = 0; i + 1 < data_appends; i += 2) {
    snprintf(buf, sizeof buf, "%s[%zu, %zu]", i ? ", " : "", sink.appends[i].first,
             sink.appends[i].second);
    blocks += buf;
  }

  Source src(sink.data);
  leveldb::Table* table = nullptr;
  if (!leveldb::Table::Open(o, &src, sink.data.size(), &table).ok()) abort();
  std::unique_ptr<leveldb::Table> owner(table);
  std::unique_ptr<leveldb::Block> index(ReadOne(src, sink.appends[ia].first, sink.appends[ia].second));
  std::vector<std::unique_ptr<leveldb::Block>> data;
  for (size_t i = 0; i + 1 < data_appends; i += 2)
    data.emplace_back(ReadOne(src, sink.appends[i].first, sink.appends[i].second));

  // the queries: the fixed ones, every index separator, and per block its
  // last key as a lookup would ask for it and a key between it and the next
  std::vector<std::string> queries = fixed_queries;
  {
    std::unique_ptr<leveldb::Iterator> it(index->NewIterator(cmp));
    for (it->SeekToFirst(); it->Valid(); it->Next()) queries.push_back(it->key().ToString());
  }
  for (const auto& blk : data) {
    std::unique_ptr<leveldb::Iterator> it(blk->NewIterator(cmp));
    it->SeekToLast();
    if (!it->Valid()) abort();
    std::string last = it->key().ToString();
    if (c.key_format == 1) {
      const std::string user = last.substr(0, last.size() - 8);
      uint64_t tag = 0;
      for (int i = 7; i >= 0; --i) tag = (tag << 8) | static_cast<unsigned char>(last[user.size() + i]);
      queries.push_back(IKey(user, tag >> 8));
      queries.push_back(IKey(user + "!", 1000));
    } else {
      queries.push_back(last);
      queries.push_back(last + "!");
    }
  }
  std::set<std::string> present;
  for (const auto& e : c.entries)
    present.insert(c.key_format == 1 ? e.first.substr(0, e.first.size() - 8) : e.first);
  // absent keys: some the filter turns away, some it lets through
  if (search_false_positives) {
    int passed = 0, turned = 0;
    for (int i = 0; i < 60 && (passed < 5 || turned < 4); ++i)
      for (int j = 0; j < 60 && (passed < 5 || turned < 4); ++j) {
        const std::string user = Num("k%04d~%d", i, j);
        if (present.count(user)) continue;
        const std::string q = c.key_format == 1 ? IKey(user, 1000) : user;
        Saved s;
        const int before = src.reads;
        if (!leveldb::TableCache::Get(table, q, &s, Save).ok()) abort();
        const bool read = src.reads != before;
        if (read && passed < 5) {
          queries.push_back(q);
          ++passed;
        } else if (!read && turned < 4) {
          queries.push_back(q);
          ++turned;
        }
      }
    if (c.filter && data.size() > 1 && passed == 0) abort();  // (the search found none)
  }

  std::string qjson;
  for (const std::string& q : queries) {
    Saved s;
    const int before = src.reads;
    const Status st = leveldb::TableCache::Get(table, q, &s, Save);
    const bool read = src.reads != before;
    std::unique_ptr<leveldb::Iterator> ii(index->NewIterator(cmp));
    ii->Seek(q);
    std::string bseek;
    for (const auto& blk : data) {
      std::unique_ptr<leveldb::Iterator> it(blk->NewIterator(cmp));
      it->Seek(q);
      bseek += std::string(bseek.empty() ? "" : ", ") + "\"" + SeekString(it.get()) + "\"";
    }
    qjson += std::string(qjson.empty() ? "" : ",\n      ") + "{\"k\": \"" + Hex(q) +
             "\", \"called\": " + (s.called ? "1" : "0") + ", \"ek\": \"" + Hex(s.key) +
             "\", \"ev\": \"" + Hex(s.value) + "\", \"st\": \"" + st.ToString() +
             "\", \"read\": " + (read ? "1" : "0") + ", \"iseek\": \"" + SeekString(ii.get()) +
             "\", \"bseek\": [" + bseek + "]}";
  }
  std::string filter = "null";
  if (c.filter) {
    snprintf(buf, sizeof buf, "[%zu, %zu]", sink.appends[fa].first, sink.appends[fa].second);
    filter = buf;
  }
  snprintf(buf, sizeof buf, "[%zu, %zu]", sink.appends[ia].first, sink.appends[ia].second);
  json += std::string(json.empty() ? "" : ",\n") + "  \"" + c.name + "\": {\"file\": \"" + file +
          "\", \"key_format\": " + std::to_string(c.key_format) + ", \"compression\": " +
          (c.snappy ? "1" : "0") + ", \"restart_interval\": " + std::to_string(c.restart_interval) +
          ", \"block_size\": " + std::to_string(c.block_size) + ", \"entries\": " +
          std::to_string(c.entries.size()) + ",\n    \"index\": " + buf + ", \"filter\": " + filter +
          ", \"blocks\": [" + blocks + "],\n    \"queries\": [\n      " + qjson + "]}";
}

// Internal keys: plain keys, one user key in several versions, a deletion as
// the newest version, user keys that are prefixes of one another.
std::vector<Entry> InternalEntries(int nplain) {
  std::vector<Entry> e;
  for (int i = 0; i < nplain; ++i) e.push_back({IKey(Num("k%04d", i), 100 + i), Val()});
  for (uint64_t seq : {50, 40, 30, 20}) e.push_back({IKey("multi", seq, seq == 30 ? 0 : 1), Val()});
  e.push_back({IKey("del", 90, 0), ""});
  e.push_back({IKey("del", 80), Val()});
  for (const char* u : {"pre", "pref", "prefix"}) e.push_back({IKey(u, 60), Val()});
  return e;
}

std::vector<std::string> InternalQueries(int nplain) {
  std::vector<std::string> q;
  q.push_back(IKey("\x01", 1000));   // before the first entry
  q.push_back(IKey("zzzz", 1000));   // after the last
  for (uint64_t seq : {1000, 50, 45, 35, 30, 25, 10}) q.push_back(IKey("multi", seq));
  for (uint64_t seq : {1000, 90, 85, 80, 5}) q.push_back(IKey("del", seq));
  for (const char* u : {"pr", "pre", "pref", "prefi", "prefix", "prefixx"}) q.push_back(IKey(u, 1000));
  for (int i = 0; i < nplain; i += 7) q.push_back(IKey(Num("k%04d", i), 1000));
  for (int i = 3; i < nplain; i += 11) q.push_back(IKey(Num("k%04d", i), 100 + i - 1));  // too old
  return q;
}

}  // namespace

int main(int argc, char** argv) {
  dir = argc > 1 ? argv[1] : ".";
  bloom = leveldb::NewBloomFilterPolicy(10);
  icmp = new leveldb::InternalKeyComparator(leveldb::BytewiseComparator());
  ipolicy = new leveldb::InternalFilterPolicy(bloom);

  Emit({"internal_bloom_r16", 1, true, false, 16, 256, InternalEntries(40)}, InternalQueries(40), true);
  Emit({"internal_plain_r2_snappy", 1, false, true, 2, 200, InternalEntries(24)}, InternalQueries(24),
       false);
  Emit({"internal_bloom_r1_snappy", 1, true, true, 1, 300, InternalEntries(24)}, InternalQueries(24),
       true);
  Emit({"one_entry", 1, true, false, 16, 4096, {{IKey("only", 7), "value"}}},
       {IKey("a", 9), IKey("only", 9), IKey("only", 7), IKey("only", 6), IKey("onlz", 9)}, false);
  Emit({"one_block_r16", 1, false, false, 16, 4096, InternalEntries(30)}, InternalQueries(30), false);
  {
    std::vector<Entry> e;
    for (int i = 0; i < 40; ++i) e.push_back({Num("b%03d", i), Val()});
    for (const char* k : {"", "a", "ab", "abc", "\xff", "\xff\xff"}) e.push_back({k, Val()});
    e.push_back({std::string("ab\0", 3), Val()});
    std::vector<std::string> q = {"", std::string("\0", 1), "a", "aa", "ab", std::string("ab\0", 3),
                                  "abb", "abc", "abd", "b", "b000", "b0000", "b017", "b039",
                                  "b0391", "c", "\xfe", "\xff", "\xff\x01", "\xff\xff", "\xff\xff\xff"};
    Emit({"bytes_r16", 0, false, false, 16, 128, e}, q, false);
    Emit({"bytes_r1_snappy", 0, false, true, 1, 160, e}, q, false);
  }
  FILE* f = fopen((dir + "/get_cases.json").c_str(), "w");
  fprintf(f, "{\n%s\n}\n", json.c_str());
  fclose(f);
  return 0;
}
