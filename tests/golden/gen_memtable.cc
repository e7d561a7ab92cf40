// Writes the memtable_*.log / .ldb / .vtb fixtures and memtable_cases.json:
// write batches, good and damaged, written through the reference's own
// log::Writer, and what the loop of DBImpl::RecoverLogFile (db/db_impl.cc:453-488)
// makes of each log with the reference's own classes -- log::Reader(checksum =
// true), WriteBatchInternal::SetContents / InsertInto, MemTable, BuildTable --
// with paranoid_checks off and on: every batch's Iterate status, the
// memtable's iteration as (batch, index) pairs with each internal key,
// max_sequence, the final status, and the tables BuildTable wrote for
// kv_sep_size 16 and for one nothing reaches. The expectation
// tests/memtable_model.py is pinned against, and
// lvkv_memtable_from_batches_device through it. TEST INFRASTRUCTURE; not part
// of the build. From the repository root, with the reference tree at $REF:
//
//   g++ -O2 -std=c++17 -DLEVELDB_PLATFORM_POSIX=1 -DLEVELDB_HAS_PORT_CONFIG_H=0 \
//       -DHAVE_SNAPPY=0 -DHAVE_ZSTD=0 -I$REF -I$REF/include -w -o /tmp/gen_memtable \
//       tests/golden/gen_memtable.cc \
//       $(ls $REF/util/*.cc $REF/table/*.cc $REF/db/*.cc | \
//         grep -v -e _test -e testutil -e env_windows -e leveldbutil -e /c.cc) -lpthread
//   /tmp/gen_memtable tests/golden
//
// The two cases the reference leaves undefined are not run: two entries with
// equal internal keys (SkipList::Insert asserts) and a user key of 2^32 - 8
// bytes (MemTable::Add truncates its length).
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "db/builder.h"
#include "db/dbformat.h"
#include "db/filename.h"
#include "db/log_reader.h"
#include "db/log_writer.h"
#include "db/memtable.h"
#include "db/table_cache.h"
#include "db/version_edit.h"
#include "db/write_batch_internal.h"
#include "leveldb/env.h"
#include "leveldb/filter_policy.h"
#include "leveldb/iterator.h"
#include "leveldb/options.h"
#include "leveldb/write_batch.h"
#include "table/vtable_format.h"

namespace {

using leveldb::Slice;
using leveldb::Status;

std::string out_dir, tmp_dir, json;
leveldb::Env* env;
const uint64_t kFileNumber = 5;

std::string Hex(const Slice& s) {
  std::string out;
  char buf[4];
  for (size_t i = 0; i < s.size(); ++i) {
    snprintf(buf, sizeof buf, "%02x", static_cast<unsigned char>(s[i]));
    out += buf;
  }
  return out;
}

void Die(const std::string& what) {
  fprintf(stderr, "gen_memtable: %s\n", what.c_str());
  exit(1);
}

std::string ReadAll(const std::string& path) {
  std::string data;
  if (!leveldb::ReadFileToString(env, path, &data).ok()) Die("cannot read " + path);
  return data;
}

void WriteAll(const std::string& path, const std::string& data) {
  if (!leveldb::WriteStringToFile(env, data, path).ok()) Die("cannot write " + path);
}

// ---- the bytes of a batch, put together by hand so that they can be wrong ----

std::string Fixed(uint64_t v, int n) {
  std::string s(n, '\0');
  for (int k = 0; k < n; ++k) s[k] = static_cast<char>(v >> (8 * k));
  return s;
}

std::string Varint(uint32_t v) {
  std::string s;
  while (v >= 128) {
    s.push_back(static_cast<char>(v | 128));
    v >>= 7;
  }
  s.push_back(static_cast<char>(v));
  return s;
}

std::string Pattern(uint32_t seed, size_t n) {
  std::string s(n, '\0');
  for (size_t j = 0; j < n; ++j) s[j] = static_cast<char>((seed * 131u + j * 7u + (j >> 8)) & 0xffu);
  return s;
}

// A value as the fork's Put leaves it in a batch: the type byte, then the bytes.
std::string Val(uint32_t seed, size_t len) {
  return len == 0 ? std::string() : std::string(1, '\x02') + Pattern(seed, len - 1);
}

std::string Put(const std::string& k, const std::string& v) {
  return std::string(1, '\x01') + Varint(k.size()) + k + Varint(v.size()) + v;
}

std::string Del(const std::string& k) { return std::string(1, '\0') + Varint(k.size()) + k; }

std::string Batch(uint64_t seq, uint32_t count, const std::string& body) {
  return Fixed(seq, 8) + Fixed(count, 4) + body;
}

// ---- RecoverLogFile's loop ---------------------------------------------------------

struct Seen : public leveldb::WriteBatch::Handler {
  std::vector<std::pair<std::string, int>> keys;  // user key, type
  void Put(const Slice& key, const Slice&) override { keys.push_back({key.ToString(), 1}); }
  void Delete(const Slice& key) override { keys.push_back({key.ToString(), 0}); }
};

struct Reporter : public leveldb::log::Reader::Reporter {
  Status* status;  // null: paranoid_checks off
  size_t calls = 0, bytes = 0;
  void Corruption(size_t n, const Status& s) override {
    ++calls;
    bytes += n;
    if (status != nullptr && status->ok()) *status = s;
  }
};

std::string Table(const std::string& name, const std::string& tag, uint64_t sep,
                  leveldb::MemTable* mem, const leveldb::InternalKeyComparator& icmp) {
  const leveldb::FilterPolicy* bloom = leveldb::NewBloomFilterPolicy(10);
  leveldb::InternalFilterPolicy ipolicy(bloom);
  leveldb::Options o;
  o.env = env;
  o.comparator = &icmp;
  o.filter_policy = &ipolicy;
  o.compression = leveldb::kNoCompression;
  o.kv_sep_size = sep;
  const std::string dbname = tmp_dir + "/" + name + "_" + tag;
  env->CreateDir(dbname);
  leveldb::TableCache cache(dbname, o, 10);
  leveldb::FileMetaData meta;
  meta.number = kFileNumber;
  leveldb::VTableMeta vmeta;
  vmeta.number = 0;
  vmeta.records_num = 0;
  vmeta.table_size = 0;
  leveldb::Iterator* it = mem->NewIterator();
  const Status s = leveldb::BuildTable(dbname, env, o, &cache, it, &meta, &vmeta);
  delete it;
  if (!s.ok()) Die(name + ": BuildTable: " + s.ToString());
  std::string j = "\"kv_sep_size\":" + std::to_string(sep);
  const std::string ldb_path = leveldb::TableFileName(dbname, kFileNumber);
  if (meta.file_size > 0 && env->FileExists(ldb_path)) {
    const std::string f = "memtable_" + name + "_" + tag + ".ldb";
    WriteAll(out_dir + "/" + f, ReadAll(ldb_path));
    j += ",\"ldb\":\"" + f + "\"";
  } else {
    j += ",\"ldb\":null";
  }
  const std::string vtb_path = leveldb::VTableFileName(dbname, kFileNumber);
  if (meta.file_size > 0 && env->FileExists(vtb_path)) {
    const std::string f = "memtable_" + name + "_" + tag + ".vtb";
    WriteAll(out_dir + "/" + f, ReadAll(vtb_path));
    j += ",\"vtb\":\"" + f + "\"";
  } else {
    j += ",\"vtb\":null";
  }
  delete bloom;
  return "{" + j + "}";
}

// One recovery of the log at `path`; ,"<mode>":{..}
std::string Recover(const std::string& name, const std::string& path, bool paranoid,
                    uint64_t max_sequence) {
  leveldb::InternalKeyComparator icmp(leveldb::BytewiseComparator());
  leveldb::SequentialFile* file;
  Status status = env->NewSequentialFile(path, &file);
  if (!status.ok()) Die("cannot open " + path);
  Reporter reporter;
  reporter.status = paranoid ? &status : nullptr;
  leveldb::log::Reader reader(file, &reporter, true, 0);
  std::string scratch;
  Slice record;
  leveldb::WriteBatch batch;
  leveldb::MemTable* mem = nullptr;
  std::map<std::string, std::pair<int, int>> where;  // internal key -> (batch, index)
  std::string statuses;
  int b = -1;
  while (reader.ReadRecord(&record, &scratch) && status.ok()) {
    ++b;
    if (!statuses.empty()) statuses += ",";
    if (record.size() < 12) {
      const Status small = Status::Corruption("log record too small");
      reporter.Corruption(record.size(), small);
      statuses += "\"" + small.ToString() + "\"";
      continue;
    }
    leveldb::WriteBatchInternal::SetContents(&batch, record);
    if (mem == nullptr) {
      mem = new leveldb::MemTable(icmp);
      mem->Ref();
    }
    {  // which (batch, index) every internal key came from
      Seen seen;
      batch.Iterate(&seen);
      const uint64_t seq = leveldb::WriteBatchInternal::Sequence(&batch);
      for (size_t j = 0; j < seen.keys.size(); ++j) {
        const std::string ikey = seen.keys[j].first + Fixed(((seq + j) << 8) | seen.keys[j].second, 8);
        if (where.count(ikey)) Die(name + ": equal internal keys are not to be run");
        where[ikey] = {b, static_cast<int>(j)};
      }
    }
    status = leveldb::WriteBatchInternal::InsertInto(&batch, mem);
    statuses += "\"" + status.ToString() + "\"";
    if (!paranoid) status = Status::OK();  // MaybeIgnoreError
    if (!status.ok()) break;
    const uint64_t last_seq = leveldb::WriteBatchInternal::Sequence(&batch) +
                              leveldb::WriteBatchInternal::Count(&batch) - 1;
    if (last_seq > max_sequence) max_sequence = last_seq;
  }
  delete file;
  std::string j = "{\"batch_status\":[" + statuses + "],\"status\":\"" + status.ToString() +
                  "\",\"max_sequence\":" + std::to_string(max_sequence) + ",\"reports\":" +
                  std::to_string(reporter.calls) + ",\"report_bytes\":" +
                  std::to_string(reporter.bytes) + ",\"entries\":[";
  if (mem != nullptr) {
    leveldb::Iterator* it = mem->NewIterator();
    bool first = true;
    for (it->SeekToFirst(); it->Valid(); it->Next()) {
      const auto at = where.find(it->key().ToString());
      if (at == where.end()) Die(name + ": an entry nobody inserted");
      j += std::string(first ? "" : ",") + "\n[" + std::to_string(at->second.first) + "," +
           std::to_string(at->second.second) + ",\"" + Hex(it->key()) + "\"]";
      first = false;
    }
    delete it;
  }
  // WriteLevel0Table (the paranoid run's tables, where it writes any, are the plain run's:
  // the same batches went into the memtable)
  const bool writes = mem != nullptr && status.ok();
  j += std::string("],\"writes_table\":") + (writes ? "true" : "false") + ",\"tables\":[";
  if (writes && !paranoid) {
    j += Table(name, "s16", 16, mem, icmp) + ",";
    j += Table(name, "big", uint64_t{1} << 40, mem, icmp);
  }
  j += "]}";
  if (mem != nullptr) mem->Unref();
  return j;
}

int ncases = 0;
void Case(const std::string& name, const std::vector<std::string>& batches,
          uint64_t max_sequence = 0) {
  const std::string path = tmp_dir + "/" + name + ".log";
  {
    leveldb::WritableFile* file;
    if (!env->NewWritableFile(path, &file).ok()) Die("cannot create " + path);
    leveldb::log::Writer writer(file);
    for (const std::string& b : batches)
      if (!writer.AddRecord(b).ok()) Die(name + ": AddRecord");
    file->Close();
    delete file;
  }
  WriteAll(out_dir + "/memtable_" + name + ".log", ReadAll(path));
  json += std::string(ncases++ ? ",\n" : "") + "\"" + name + "\":{\"log\":\"memtable_" + name +
          ".log\",\"nbatches\":" + std::to_string(batches.size()) + ",\"max_sequence_in\":" +
          std::to_string(max_sequence) + ",\n\"plain\":" + Recover(name, path, false, max_sequence) +
          ",\n\"paranoid\":" + Recover(name, path, true, max_sequence) + "}";
}

std::string Key(int i) {
  char key[16];
  snprintf(key, sizeof key, "key%05d", i);
  return key;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) Die("usage: gen_memtable <output directory>");
  out_dir = argv[1];
  env = leveldb::Env::Default();
  char tmpl[] = "/tmp/gen_memtable_XXXXXX";
  if (mkdtemp(tmpl) == nullptr) Die("mkdtemp");
  tmp_dir = tmpl;
  json = "{\n";

  {  // batches of 0, 1, 2 and 65 entries; records of 0, 11 and 12 bytes
    std::string b65;
    for (int i = 0; i < 65; ++i)
      b65 += i % 7 == 3 ? Del(Key(200 - i)) : Put(Key(200 - i), Val(i, i % 5 == 0 ? 40 : 3 + i % 9));
    Case("sizes", {Batch(10, 0, ""), Batch(10, 1, Put("one", Val(1, 5))), std::string(),
                   Batch(11, 2, Put("two_a", Val(2, 20)) + Del("two_b")), std::string(11, '\x01'),
                   Batch(13, 65, b65), Batch(78, 0, "")});
    Case("empty_count_0", {Batch(5, 0, "")});
    Case("empty_count_1", {Batch(5, 1, "")});
    Case("only_small", {std::string(), std::string(11, '\0')}, 77);
  }
  {  // one user key put and deleted across four batches and inside one
    Case("versions",
         {Batch(100, 2, Put("k", Val(1, 10)) + Put("j", Val(2, 30))), Batch(102, 1, Del("k")),
          Batch(103, 3, Put("k", Val(3, 17)) + Del("k") + Put("k", Val(4, 2))),
          Batch(106, 2, Put("l", Val(5, 16)) + Put("k", Val(6, 15)))});
  }
  {  // user keys of 0, 1, 7, 8, 9 and 300 bytes; ties on the first 8 bytes
    const std::string long_a = std::string(299, 'q') + "a", long_b = std::string(299, 'q') + "b";
    std::string body;
    const std::vector<std::string> keys = {
        long_b, "", "a", "abcdefg", "abcdefgh", "abcdefghi", "abcdefghj", long_a,
        std::string("ab\0", 3), "ab", std::string("abcdefgh\0", 9), "\x7f", "\x80", "\xff",
        std::string("\0", 1), std::string("\xff\xff\xff\xff\xff\xff\xff\xff", 8),
        std::string("\xff\xff\xff\xff\xff\xff\xff\xff\x01", 9)};
    for (size_t i = 0; i < keys.size(); ++i) body += Put(keys[i], Val(i, 4 + 3 * i));
    Case("keys", {Batch(1000, keys.size(), body)});
  }
  {  // already sorted, reverse sorted and shuffled input
    std::string up, down, mixed[2];
    for (int i = 0; i < 24; ++i) {
      up += Put(Key(i), Val(i, 8 + i));
      down += Put(Key(23 - i), Val(i, 8 + i));
      mixed[i / 12] += Put(Key(i * 7 % 24), Val(i, 8 + i));
    }
    Case("sorted", {Batch(1, 24, up)});
    Case("reversed", {Batch(1, 24, down)});
    Case("shuffled", {Batch(1, 12, mixed[0]), Batch(13, 12, mixed[1])});
  }
  {  // varints: five bytes for a small length; cut by the batch's end; one past the end
    const std::string five = std::string("\x83\x80\x80\x80\x00", 5);  // 3
    const std::string five_high = std::string("\x83\x80\x80\x80\x70", 5);  // 3 and bits past 32
    Case("varint_five_bytes",
         {Batch(1, 2, std::string(1, '\x01') + five + "abc" + five + "\x02xy" +
                          std::string(1, '\0') + five_high + "abd")});
    Case("varint_cut", {Batch(1, 2, Put("a", Val(1, 3)) + std::string("\x01\x80", 2))});
    Case("varint_cut_value", {Batch(1, 1, std::string("\x01\x01k\x80\x80", 5))});
    Case("varint_six_bytes", {Batch(1, 1, std::string("\x00\x80\x80\x80\x80\x80\x00", 7))});
    Case("length_past_end", {Batch(1, 2, Put("a", Val(1, 3)) + std::string("\x01\x02k", 3))});
    Case("value_past_end", {Batch(1, 1, std::string("\x01\x01k\x03\x02x", 6))});
    Case("no_value", {Batch(1, 1, std::string("\x01\x01k", 3))});
  }
  {  // a bad tag, a failing put, a failing delete: in the first, a middle and the last batch,
     // at the first, a middle and the last record
    const std::string bad[3] = {std::string("\x02\x01k", 3), std::string("\x01\x05k", 3),
                                std::string("\x00\x05k", 3)};
    const char* kind[3] = {"tag", "put", "delete"};
    const char* where[3] = {"first", "middle", "last"};
    for (int k = 0; k < 3; ++k) {
      std::vector<std::string> all;
      for (int bpos = 0; bpos < 3; ++bpos) {
        std::vector<std::string> batches;
        for (int b = 0; b < 3; ++b) {
          const int rpos = (bpos + k) % 3;
          std::string body;
          for (int r = 0; r < 3; ++r) {
            if (b == bpos && r == rpos) {
              body += bad[k];
              break;  // (what follows a failing record is never looked at; a bad tag's rest is)
            }
            body += r == 1 ? Del(Key(10 * b + r)) : Put(Key(10 * b + r), Val(b + r, 6));
          }
          if (b == bpos && rpos != 2 && k == 0) body += Put(Key(99), Val(9, 9));
          batches.push_back(Batch(50 + 3 * b, 3, body));
          if (b == bpos) all.push_back(Batch(50 + 3 * all.size(), 3, body));
        }
        Case(std::string("bad_") + kind[k] + "_" + where[bpos], batches);
      }
      Case(std::string("bad_") + kind[k] + "_all", all);
    }
    for (int bpos = 0; bpos < 3; ++bpos) {
      for (int d = -1; d <= 1; d += 2) {
        std::vector<std::string> batches;
        for (int b = 0; b < 3; ++b)
          batches.push_back(Batch(50 + 3 * b, b == bpos ? 2 + d : 2,
                                  Put(Key(10 * b), Val(b, 12)) + Del(Key(10 * b + 1))));
        Case(std::string("count_") + (d < 0 ? "fewer_" : "more_") + where[bpos], batches);
      }
    }
  }
  {  // the trailer wraps; count as a negative int
    const uint64_t seq = (uint64_t{1} << 56) - 2;
    Case("sequence_wraps", {Batch(seq, 4, Put("a", Val(1, 5)) + Put("b", Val(2, 5)) +
                                              Put("c", Val(3, 5)) + Del("d"))});
    Case("count_negative", {Batch(100, 0x80000000u, ""), Batch(7, 1, Put("a", Val(1, 5)))});
  }
  {  // a batch that spans three 32 KiB log blocks
    Case("three_blocks", {Batch(1, 1, Put("before", Val(1, 9))),
                          Batch(2, 3, Put("big_a", Val(2, 33000)) + Del("gone") +
                                          Put("big_b", Val(3, 33000))),
                          Batch(5, 1, Put("after", Val(4, 9)))});
  }
  json += "\n}\n";
  WriteAll(out_dir + "/memtable_cases.json", json);
  return 0;
}
