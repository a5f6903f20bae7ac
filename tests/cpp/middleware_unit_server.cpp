// The native Middleware server (host/ipls_middleware.hpp) with unit updates
// switched on, for tests/test_middleware_unit.py to drive as a client:
//   middleware_unit_server P MIN_PEERS CONNECTIONS CHUNK [IO_TIMEOUT_MS]
// Prints "port N" once it listens.  A task that fails prints "error TASK",
// then the state a broken task 2 must leave untouched: "pending N" and, per
// partition, "agg P CHECKSUM" (ipls_agg_checksum of Aggregated_Gradients).
// Prints "done ROUNDS FAILED" after the last connection and exits 0.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "ipls_middleware.hpp"

int main(int argc, char** argv) {
  if (argc != 5 && argc != 6) {
    std::fprintf(stderr, "usage: %s partitions min_peers connections chunk [io_timeout_ms]\n", argv[0]);
    return 2;
  }
  ipls_host::PeerData opts;
  opts._PARTITIONS = std::atoi(argv[1]);
  opts.Min_Members = std::atoi(argv[2]);
  const int connections = std::atoi(argv[3]);
  ipls_host::MiddlewareServer server(opts, std::atoll(argv[4]), argc == 6 ? std::atoi(argv[5]) : 30000,
                                     /*unit_updates=*/true);
  std::printf("port %d\n", server.listen(0));
  std::fflush(stdout);
  server.serve(connections, [&](int16_t task, const ipls_host::JavaException&) {
    std::printf("error %d\npending %d\n", (int)task, server.pending());
    if (server.ipls())
      for (int p = 0; p < opts._PARTITIONS; ++p) {
        uint64_t c = 0;
        if (ipls_agg_checksum(server.ipls()->handle(), p, IPLS_TGT_AGG, &c) != 0) return;
        std::printf("agg %d %" PRIu64 "\n", p, c);
      }
    std::fflush(stdout);
  });
  std::printf("done %" PRId64 " %" PRId64 "\n", server.stats().rounds, server.stats().failed);
  return 0;
}
