// h2dbench: what is the fastest way to move pinned host bytes into HBM on this
// GPU? The staging step (host tier -> HBM) bounds the 1-GPU headline and, at 8
// GPUs, each GPU's share of the layers that must cross PCIe once.
//
//   bin/h2dbench [-gib N] [-device D] [-paths sdma,kernel,pageable,bounce]
//
// Compares, over N GiB of pinned host memory (hipHostMalloc):
//  * hipMemcpyAsync (SDMA copy engine) in chunks of 4-256 MiB on 1, 2 and 4 streams;
//  * a gfx950 copy kernel that reads the host buffer directly over PCIe
//    (host-mapped pointer, 16 B per lane, non-temporal), at several grid sizes;
//  * SDMA + kernel together (half the chunks each);
// and, for host layers that did not fit the pinned pool, over N GiB of
// pageable memory (posix_memalign) and the same chunk sizes:
//  * "pageable": hipMemcpyAsync straight from it on 2 streams (the runtime
//    stages the bytes itself and the call blocks meanwhile);
//  * "bounce": T = 1, 2, 4, 8 host threads memcpy chunks into a ring of 8
//    pinned buffers, each followed by an H2D copy on a stream of its own - the
//    engine's path for such layers (engine/planned_stage.cc);
//  * "bounce+pinned": the same beside pinned copies on two other streams,
//    pageable to pinned bytes 1 : 4 (N / 4 GiB through the ring, N GiB pinned):
//    GBps is all bytes over the time until both are done, bounce_GBps the
//    ring's bytes over the time until the ring's last copy landed.
// Prints one JSON line per configuration.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#define CHECK(x)                                                       \
  do {                                                                 \
    hipError_t err_ = (x);                                             \
    if (err_ != hipSuccess) {                                          \
      fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(err_)); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

using u32x4 = unsigned int __attribute__((ext_vector_type(4)));

// Grid-stride copy, 16 B per lane; reads cross PCIe (host-mapped source).
__global__ void __launch_bounds__(256) pull_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst,
                                                   int64_t n16) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  // 4 loads in flight per lane before the stores.
  for (; i + 3 * stride < n16; i += 4 * stride) {
    u32x4 a = __builtin_nontemporal_load(src + i);
    u32x4 b = __builtin_nontemporal_load(src + i + stride);
    u32x4 c = __builtin_nontemporal_load(src + i + 2 * stride);
    u32x4 d = __builtin_nontemporal_load(src + i + 3 * stride);
    __builtin_nontemporal_store(a, dst + i);
    __builtin_nontemporal_store(b, dst + i + stride);
    __builtin_nontemporal_store(c, dst + i + 2 * stride);
    __builtin_nontemporal_store(d, dst + i + 3 * stride);
  }
  for (; i < n16; i += stride) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// `threads` host threads move [src, src + bytes) to dst in chunks through a
// ring of pinned buffers: take a buffer, wait for the H2D copy last issued from
// it, memcpy the next chunk in, issue its H2D copy on `stream`. Returns once
// every copy is issued; the caller synchronizes `stream`.
static void bounce_copy(int device, int threads, const uint8_t* src, uint8_t* dst, int64_t bytes, int64_t chunk,
                        const std::vector<uint8_t*>& ring, const std::vector<hipEvent_t>& landed, hipStream_t stream) {
  std::mutex mu;  // the free list, and the order of copy + event on the stream
  std::condition_variable cv;
  std::deque<int> free_bufs;
  for (int i = 0; i < int(ring.size()); ++i) free_bufs.push_back(i);
  std::atomic<int64_t> next{0};
  std::vector<std::thread> ths;
  for (int t = 0; t < threads; ++t)
    ths.emplace_back([&] {
      CHECK(hipSetDevice(device));
      for (;;) {
        const int64_t off = next.fetch_add(chunk);
        if (off >= bytes) return;
        const int64_t len = std::min(chunk, bytes - off);
        int b;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return !free_bufs.empty(); });
          b = free_bufs.front();
          free_bufs.pop_front();
        }
        CHECK(hipEventSynchronize(landed[size_t(b)]));
        memcpy(ring[size_t(b)], src + off, size_t(len));
        {
          std::lock_guard<std::mutex> lk(mu);
          CHECK(hipMemcpyAsync(dst + off, ring[size_t(b)], size_t(len), hipMemcpyHostToDevice, stream));
          CHECK(hipEventRecord(landed[size_t(b)], stream));
          free_bufs.push_back(b);
        }
        cv.notify_one();
      }
    });
  for (auto& th : ths) th.join();
}

int main(int argc, char** argv) {
  int64_t gib = 4;
  int device = 0;
  std::string paths = "sdma,kernel,pageable,bounce";
  for (int i = 1; i + 1 < argc; i += 2) {
    std::string a = argv[i];
    if (a == "-gib") gib = atoll(argv[i + 1]);
    else if (a == "-device") device = atoi(argv[i + 1]);
    else if (a == "-paths") paths = argv[i + 1];
  }
  auto wanted = [&](const char* p) { return ("," + paths + ",").find(std::string(",") + p + ",") != std::string::npos; };
  CHECK(hipSetDevice(device));
  const int64_t n = gib << 30;
  uint8_t *host = nullptr, *dev = nullptr, *hdev = nullptr;
  CHECK(hipHostMalloc(reinterpret_cast<void**>(&host), size_t(n), hipHostMallocMapped));
  CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&hdev), host, 0));
  CHECK(hipMalloc(&dev, size_t(n)));
  for (int64_t i = 0; i < n; i += 4096) host[i] = uint8_t(i >> 12);
  std::vector<hipStream_t> st(4);
  for (auto& s : st) CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

  auto report = [&](const char* what, int64_t chunk_mib, int streams, int blocks, double sec) {
    printf("{\"path\": \"%s\", \"chunk_mib\": %lld, \"streams\": %d, \"blocks\": %d, \"GBps\": %.2f}\n", what,
           (long long)chunk_mib, streams, blocks, double(n) / sec / 1e9);
    fflush(stdout);
  };
  auto sync_all = [&] {
    for (auto& s : st) CHECK(hipStreamSynchronize(s));
  };
  auto best_of = [&](auto&& run) {
    run();  // warm
    sync_all();
    double best = 1e9;
    for (int r = 0; r < 3; ++r) {
      double t0 = now();
      run();
      sync_all();
      best = std::min(best, now() - t0);
    }
    return best;
  };

  for (int64_t cm : {4, 16, 64, 256}) {
    for (int ns : {1, 2, 4}) {
      if (!wanted("sdma")) break;
      const int64_t chunk = cm << 20;
      double t = best_of([&] {
        int k = 0;
        for (int64_t off = 0; off < n; off += chunk, ++k)
          CHECK(hipMemcpyAsync(dev + off, host + off, size_t(std::min(chunk, n - off)), hipMemcpyHostToDevice,
                               st[size_t(k % ns)]));
      });
      report("sdma", cm, ns, 0, t);
    }
  }
  for (int blocks : {64, 128, 256, 512, 1024, 2048}) {
    if (!wanted("kernel")) break;
    double t = best_of([&] {
      pull_kernel<<<blocks, 256, 0, st[0]>>>(reinterpret_cast<const u32x4*>(hdev), reinterpret_cast<u32x4*>(dev),
                                             n / 16);
      CHECK(hipGetLastError());
    });
    report("kernel_pull", 0, 1, blocks, t);
  }
  for (int blocks : {128, 512}) {
    if (!wanted("kernel")) break;
    // Interleaved 64 MiB chunks: even ones on SDMA, odd ones pulled by the kernel.
    const int64_t chunk = 64ll << 20;
    double t = best_of([&] {
      int k = 0;
      for (int64_t off = 0; off < n; off += chunk, ++k) {
        const int64_t len = std::min(chunk, n - off);
        if (k % 2 == 0) {
          CHECK(hipMemcpyAsync(dev + off, host + off, size_t(len), hipMemcpyHostToDevice, st[1]));
        } else {
          pull_kernel<<<blocks, 256, 0, st[0]>>>(reinterpret_cast<const u32x4*>(hdev + off),
                                                 reinterpret_cast<u32x4*>(dev + off), len / 16);
          CHECK(hipGetLastError());
        }
      }
    });
    report("sdma+kernel", 64, 2, blocks, t);
  }
  // Check the bytes arrived.
  std::vector<uint8_t> back(4096);
  auto check_tail = [&](const uint8_t* d, int64_t bytes) {
    CHECK(hipMemcpy(back.data(), d + (bytes - 4096), 4096, hipMemcpyDeviceToHost));
    if (back[0] != uint8_t((bytes - 4096) >> 12)) {
      fprintf(stderr, "data mismatch\n");
      exit(1);
    }
  };
  if (wanted("sdma") || wanted("kernel")) check_tail(dev, n);
  if (!wanted("pageable") && !wanted("bounce")) return 0;

  // ---- pageable host memory
  uint8_t* page = nullptr;
  if (posix_memalign(reinterpret_cast<void**>(&page), 4096, size_t(n)) != 0) {
    fprintf(stderr, "posix_memalign failed\n");
    return 1;
  }
  for (int64_t i = 0; i < n; i += 4096) page[i] = uint8_t(i >> 12);
  if (wanted("pageable")) {
    for (int64_t cm : {4, 16, 64, 256}) {
      const int64_t chunk = cm << 20;
      CHECK(hipMemset(dev, 0, size_t(n)));
      double t = best_of([&] {
        int k = 0;
        for (int64_t off = 0; off < n; off += chunk, ++k)
          CHECK(hipMemcpyAsync(dev + off, page + off, size_t(std::min(chunk, n - off)), hipMemcpyHostToDevice,
                               st[size_t(k % 2)]));
      });
      report("pageable", cm, 2, 0, t);
      check_tail(dev, n);
    }
  }
  if (wanted("bounce")) {
    const int kRing = 8;
    hipStream_t bs = nullptr;
    CHECK(hipStreamCreateWithFlags(&bs, hipStreamNonBlocking));
    uint8_t* dev2 = nullptr;  // the ring's landing beside pinned copies into `dev`
    CHECK(hipMalloc(&dev2, size_t(n / 4)));
    std::vector<hipEvent_t> landed(kRing);
    for (auto& e : landed) CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (int64_t cm : {4, 16, 64, 256}) {
      const int64_t chunk = cm << 20;
      std::vector<uint8_t*> ring(kRing);
      for (auto& b : ring) CHECK(hipHostMalloc(reinterpret_cast<void**>(&b), size_t(chunk), hipHostMallocDefault));
      for (int threads : {1, 2, 4, 8}) {
        CHECK(hipMemset(dev, 0, size_t(n)));
        double t = best_of([&] {
          bounce_copy(device, threads, page, dev, n, chunk, ring, landed, bs);
          CHECK(hipStreamSynchronize(bs));
        });
        printf("{\"path\": \"bounce\", \"chunk_mib\": %lld, \"threads\": %d, \"ring\": %d, \"GBps\": %.2f}\n",
               (long long)cm, threads, kRing, double(n) / t / 1e9);
        fflush(stdout);
        check_tail(dev, n);
        // beside pinned copies on two streams, pageable : pinned = 1 : 4
        CHECK(hipMemset(dev2, 0, size_t(n / 4)));
        double bounce_s = 0;
        t = best_of([&] {
          const double t0 = now();
          std::thread ring_thread([&] {
            CHECK(hipSetDevice(device));
            bounce_copy(device, threads, page, dev2, n / 4, chunk, ring, landed, bs);
            CHECK(hipStreamSynchronize(bs));
            bounce_s = now() - t0;
          });
          int k = 0;
          for (int64_t off = 0; off < n; off += chunk, ++k)
            CHECK(hipMemcpyAsync(dev + off, host + off, size_t(std::min(chunk, n - off)), hipMemcpyHostToDevice,
                                 st[size_t(k % 2)]));
          ring_thread.join();
        });
        printf("{\"path\": \"bounce+pinned\", \"chunk_mib\": %lld, \"threads\": %d, \"ring\": %d, \"GBps\": %.2f, "
               "\"bounce_GBps\": %.2f}\n",
               (long long)cm, threads, kRing, double(n + n / 4) / t / 1e9, double(n / 4) / bounce_s / 1e9);
        fflush(stdout);
        check_tail(dev2, n / 4);
      }
      for (auto& b : ring) CHECK(hipHostFree(b));
    }
  }
  return 0;
}
