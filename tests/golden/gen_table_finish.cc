// Writes the finish_*.sst fixtures and finish_tables.json: whole tables by the
// reference's TableBuilder, with Flush() where a case needs a block boundary,
// and for each the options and the data blocks' handles and types (what
// tests/sst_finish_model.py and lvkv_sst_write_table_device rebuild them
// from). TEST INFRASTRUCTURE; not part of the build. From the repository
// root, with the reference tree at $REF and libsnappy 1.1.8 under $SNAPPY
// (its include/ and lib/; the library is named by its path and libstdc++
// linked statically, because that lib/ may hold an older libstdc++ too):
//
//   g++ -O2 -std=c++17 -static-libstdc++ -DLEVELDB_PLATFORM_POSIX=1 \
//       -DLEVELDB_HAS_PORT_CONFIG_H=0 -DHAVE_SNAPPY=1 -I$REF -I$REF/include \
//       -I$SNAPPY/include -w -o /tmp/gen_table_finish tests/golden/gen_table_finish.cc \
//       $REF/util/{crc32c,coding,comparator,options,status,env,env_posix,logging,bloom,hash,filter_policy}.cc \
//       $REF/table/{table_builder,block_builder,filter_block,format}.cc $REF/db/dbformat.cc \
//       $SNAPPY/lib/libsnappy.so.1.1.8 -Wl,-rpath,$SNAPPY/lib -lpthread
//   /tmp/gen_table_finish tests/golden
#include <cstdio>
#include <string>
#include <vector>

#include "db/dbformat.h"
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/filter_policy.h"
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

struct Case {
  std::string name;
  int key_format, bits_per_key, compression, block_size;
  Sink sink;
  size_t data_appends = 0;  // appends before Finish(): two a data block
};

std::string json;

void Emit(Case& c) {
  FILE* f = fopen((c.name + ".sst").c_str(), "wb");
  fwrite(c.sink.data.data(), 1, c.sink.data.size(), f);
  fclose(f);
  char buf[256];
  snprintf(buf, sizeof buf,
           "%s  \"%s\": {\"key_format\": %d, \"bits_per_key\": %d, \"compression\": %d, "
           "\"block_size\": %d, \"file_bytes\": %zu, \"blocks\": [",
           json.empty() ? "" : ",\n", c.name.substr(c.name.rfind('/') + 1).c_str(), c.key_format,
           c.bits_per_key, c.compression, c.block_size, c.sink.data.size());
  json += buf;
  for (size_t i = 0; i + 1 < c.data_appends; i += 2) {
    const auto& a = c.sink.appends[i];
    snprintf(buf, sizeof buf, "%s{\"offset\": %zu, \"size\": %zu, \"type\": %d}", i ? ", " : "",
             a.first, a.second, c.sink.data[a.first + a.second]);
    json += buf;
  }
  json += "]}";
}

void Finish(Case& c, leveldb::TableBuilder& b) {
  b.Flush();
  c.data_appends = c.sink.appends.size();
  b.Finish();
  Emit(c);
}

std::string IKey(const std::string& user, uint64_t seq) {
  return leveldb::InternalKey(user, seq, leveldb::kTypeValue).Encode().ToString();
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const leveldb::FilterPolicy* bloom = leveldb::NewBloomFilterPolicy(10);

  {  // internal keys, snappy, small blocks that share filters
    Case c{dir + "/finish_internal_snappy", 1, 10, 1, 1024};
    leveldb::InternalKeyComparator icmp(leveldb::BytewiseComparator());
    leveldb::InternalFilterPolicy ipolicy(bloom);
    leveldb::Options o;
    o.comparator = &icmp;
    o.filter_policy = &ipolicy;
    o.compression = leveldb::kSnappyCompression;
    o.block_size = c.block_size;
    leveldb::TableBuilder b(o, &c.sink);
    for (int i = 0; i < 300; ++i) {
      char key[32];
      snprintf(key, sizeof key, "user%06d", i * 7);
      std::string value;
      for (int j = 0; j < 6 + i % 5; ++j) value += "value-of-" + std::string(key) + ";";
      if (i == 150) {  // one user key at two sequence numbers, a block apart
        b.Add(IKey(key, 2000), value);
        b.Flush();
        b.Add(IKey(key, 1000), value);
        continue;
      }
      b.Add(IKey(key, 100 + i), value);
    }
    Finish(c, b);
  }
  {  // separator and filter edge cases, bytewise keys
    Case c{dir + "/finish_edges", 0, 10, 0, 1 << 20};
    leveldb::Options o;
    o.filter_policy = bloom;
    o.compression = leveldb::kNoCompression;
    o.block_size = c.block_size;
    leveldb::TableBuilder b(o, &c.sink);
    b.Add(std::string("aa\x01"), "v0");  // | "aa\x02": diff + 1 == limit, unchanged
    b.Flush();
    b.Add(std::string("aa\x02"), "v1");
    b.Add(std::string("ab\x01x"), "v2");  // | "ab\x05": becomes "ab\x02"
    b.Flush();
    b.Add(std::string("ab\x05"), "v3");
    b.Add("abc", "v4");  // | "abcd": a prefix, unchanged
    b.Flush();
    b.Add("abcd", "v5");
    b.Add(std::string("a\xffz"), "v6");  // | "b": 'a' + 1 == 'b', unchanged
    b.Flush();
    b.Add("b", "one entry");
    b.Flush();
    b.Add("big", std::string(10240, 'x'));  // leaves empty filters; | "d1": becomes "c"
    b.Flush();
    for (int i = 1; i < 40; ++i) {
      char key[8];
      snprintf(key, sizeof key, "d%02d", i);
      b.Add(key, std::string(i, 'y'));
      if (i % 9 == 0) b.Flush();
    }
    b.Flush();
    b.Add(std::string("\xff\xff\xff"), "last");  // no successor: unchanged
    Finish(c, b);
  }
  {  // no filter policy: an empty metaindex block
    Case c{dir + "/finish_nofilter", 0, 0, 0, 256};
    leveldb::Options o;
    o.compression = leveldb::kNoCompression;
    o.block_size = c.block_size;
    leveldb::TableBuilder b(o, &c.sink);
    for (int i = 0; i < 50; ++i) {
      char key[16], value[32];
      snprintf(key, sizeof key, "key%04d", i * 3);
      snprintf(value, sizeof value, "value%d", i * i);
      b.Add(key, value);
    }
    Finish(c, b);
  }
  {  // Finish() of a builder nothing was added to
    Case c{dir + "/finish_empty", 0, 10, 0, 4096};
    leveldb::Options o;
    o.filter_policy = bloom;
    o.compression = leveldb::kNoCompression;
    leveldb::TableBuilder b(o, &c.sink);
    Finish(c, b);
  }
  FILE* f = fopen((dir + "/finish_tables.json").c_str(), "w");
  fprintf(f, "{\n%s\n}\n", json.c_str());
  fclose(f);
  delete bloom;
  return 0;
}
