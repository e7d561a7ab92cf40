// Writes the cuts_*.sst fixtures and block_cuts.json: whole uncompressed
// tables by the reference's TableBuilder, fed with Add() alone -- the only
// Flush() is the one Finish() makes -- so that every block boundary is one
// TableBuilder chose. For each: block_size, restart_interval, key_format and
// the data blocks' handles (what tests/sst_build_model.py and
// lvkv_sst_build_blocks_device re-cut them from; the entries are read back
// out of the images' own data blocks). TEST INFRASTRUCTURE; not part of the
// build. From the repository root, with the reference tree at $REF:
//
//   g++ -O2 -std=c++17 -DLEVELDB_PLATFORM_POSIX=1 -DLEVELDB_HAS_PORT_CONFIG_H=0 \
//       -I$REF -I$REF/include -w -o /tmp/gen_block_cuts tests/golden/gen_block_cuts.cc \
//       $REF/util/{crc32c,coding,comparator,options,status,env,env_posix,logging,bloom,hash,filter_policy}.cc \
//       $REF/table/{table_builder,block_builder,filter_block,format}.cc $REF/db/dbformat.cc \
//       -lpthread
//   /tmp/gen_block_cuts tests/golden
#include <cstdio>
#include <string>
#include <vector>

#include "db/dbformat.h"
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/options.h"
#include "leveldb/table_builder.h"

namespace {

// The file as a string, and where every Append began and how long it was:
// WriteRawBlock appends a block's contents, then its 5-byte trailer.
class Sink : public leveldb::WritableFile {
 public:
  leveldb::Status Append(const leveldb::Slice& d) override {
    appends.push_back({data.size(), d.size()});
    data.append(d.data(), d.size());
    return leveldb::Status::OK();
  }
  leveldb::Status Close() override { return leveldb::Status::OK(); }
  leveldb::Status Flush() override { return leveldb::Status::OK(); }
  leveldb::Status Sync() override { return leveldb::Status::OK(); }
  std::string data;
  std::vector<std::pair<size_t, size_t>> appends;
};

typedef std::vector<std::pair<std::string, std::string>> Entries;

std::string dir, json;
const leveldb::InternalKeyComparator icmp(leveldb::BytewiseComparator());

void Table(const std::string& name, int block_size, int restart_interval, int key_format,
           const Entries& entries) {
  Sink sink;
  leveldb::Options o;
  if (key_format == 1) o.comparator = &icmp;
  o.compression = leveldb::kNoCompression;
  o.block_size = block_size;
  o.block_restart_interval = restart_interval;
  leveldb::TableBuilder b(o, &sink);
  for (const auto& e : entries) b.Add(e.first, e.second);
  b.Finish();
  FILE* f = fopen((dir + "/cuts_" + name + ".sst").c_str(), "wb");
  fwrite(sink.data.data(), 1, sink.data.size(), f);
  fclose(f);
  char buf[256];
  snprintf(buf, sizeof buf,
           "%s  \"%s\": {\"block_size\": %d, \"restart_interval\": %d, \"key_format\": %d, "
           "\"file_bytes\": %zu, \"blocks\": [",
           json.empty() ? "" : ",\n", name.c_str(), block_size, restart_interval, key_format,
           sink.data.size());
  json += buf;
  // without a filter policy Finish() ends with the metaindex block, the index
  // block (two appends each) and the footer: everything before is data blocks
  for (size_t i = 0; i + 5 < sink.appends.size(); i += 2) {
    snprintf(buf, sizeof buf, "%s{\"offset\": %zu, \"size\": %zu}", i ? ", " : "",
             sink.appends[i].first, sink.appends[i].second);
    json += buf;
  }
  json += "]}";
}

std::string Key(const char* fmt, int i) {
  char buf[64];
  snprintf(buf, sizeof buf, fmt, i);
  return buf;
}

std::string IKey(const std::string& user, uint64_t seq) {
  return leveldb::InternalKey(user, seq, leveldb::kTypeValue).Encode().ToString();
}

// Keys with long common prefixes and values of 0..36 bytes: blocks of uneven
// entry counts, few of them a multiple of any interval.
Entries Mixed(int n) {
  Entries e;
  for (int i = 0; i < n; ++i)
    e.push_back({Key("key%05d", i * 7), std::string((i * 13) % 37, 'a' + i % 26)});
  return e;
}

}  // namespace

int main(int argc, char** argv) {
  dir = argc > 1 ? argv[1] : ".";

  // the restart interval: restarts are counted from the block's first entry
  Table("r1", 128, 1, 0, Mixed(60));
  Table("r2", 128, 2, 0, Mixed(60));
  Table("r3", 160, 3, 0, Mixed(90));
  Table("r16", 700, 16, 0, Mixed(300));
  Table("rbig", 300, 1000, 0, Mixed(120));  // an interval no block reaches

  {  // the >=: with interval 1 an entry of a 5-byte key and a v-byte value
     // takes 3 + 5 + v bytes and a restart. 4 + 3 * 32 = 100 cuts after three
     // entries; 4 + 32 + 32 + 31 = 99 does not, and a fourth joins.
    Entries e;
    const int v[] = {20, 20, 20, 20, 20, 19, 20, 20, 20, 20, 7, 7};
    for (int i = 0; i < 12; ++i) e.push_back({Key("k%04d", i), std::string(v[i], 'e')});
    Table("exact_r1", 100, 1, 0, e);
  }
  {  // the same under interval 16 with keys that share nothing: 8 + v bytes an
     // entry, one restart. 8 + 4 * 23 = 100; 8 + 3 * 23 + 22 = 99.
    Entries e;
    const int v[] = {15, 15, 15, 15, 15, 15, 15, 14, 15, 15, 15, 15, 15, 3};
    for (int i = 0; i < 14; ++i) {
      std::string k = "?key!";
      k[0] = 'A' + i;
      e.push_back({k, std::string(v[i], 'x')});
    }
    Table("exact_r16", 100, 16, 0, e);
  }
  {  // values larger than block_size, several in a row: one-entry blocks
    Entries e;
    const int v[] = {10, 12, 300, 1000, 257, 400, 9, 11, 256, 5, 700, 701, 8};
    for (int i = 0; i < 13; ++i) e.push_back({Key("big%03d", i), std::string(v[i], 'B')});
    Table("bigvalues", 256, 16, 0, e);
  }
  {  // two-byte shared and non_shared varints, a three-byte value length, an empty value
    Entries e;
    e.push_back({"a-short-key", "first"});
    const std::string prefix(130, 'p');
    for (int i = 0; i < 40; ++i)
      e.push_back({prefix + Key("%04d", i), i == 7 ? std::string() : std::string(i, 'v')});
    e.push_back({std::string(200, 'q'), std::string(16500, 'L')});
    e.push_back({std::string(200, 'q') + "r", ""});
    for (int i = 0; i < 20; ++i) e.push_back({Key("zz%03d", i), "tail"});
    Table("varints", 4096, 16, 0, e);
  }
  {  // internal keys; one user key at two sequence numbers
    Entries e;
    for (int i = 0; i < 80; ++i) {
      const std::string user = Key("user%04d", i * 3);
      if (i % 11 == 5) e.push_back({IKey(user, 5000 + i), "newer-" + user});
      e.push_back({IKey(user, 100 + i), std::string(i % 19, 'i') + user});
    }
    Table("internal", 200, 4, 1, e);
  }

  FILE* f = fopen((dir + "/block_cuts.json").c_str(), "w");
  fprintf(f, "{\n%s\n}\n", json.c_str());
  fclose(f);
  return 0;
}
