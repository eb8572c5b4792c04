// Multi-GPU frames behind the C ABI (include/mirt.h, mirt_multi_*): the image-stripe data parallelism of SURVEY.md 8e in one
// process.  The scene is uploaded to every device and every device builds the identical LBVH (deterministic: no broadcast; the
// devices build concurrently, one host thread each); the frame is cut into interleaved row stripes (MirtRenderParams); device
// r renders part r into a compact buffer; the parts are gathered to device 0 with grouped RCCL send/recv over xGMI (<= 1.04 MB
// per device at 1080p, each peer on its own link) and scattered into the row-major frame there.
//
// Frames are pipelined: mirt_multi_submit issues a frame and returns, mirt_multi_wait collects it; up to
// MIRT_MULTI_MAX_IN_FLIGHT frames may be in flight, each on its own set of render streams (a scene keeps as many render
// workspaces), so that the next frame's waves move into the wave slots the draining frame frees -- on a stripe share of a
// frame the drain is a third of the time.  The gathers run in submission order on one communication stream per device (RCCL
// wants the calls on a communicator issued in one order).  One host thread drives all devices; every call is asynchronous on
// its device's streams.  The reference is single-GPU (main.cu:25-94); this replaces nothing in it.
//
// RCCL is loaded at run time (dlopen) and only when more than one device is used: libmirt.so has no link-time dependency on
// it, and a process that already holds an RCCL (PyTorch's) shares that one.  MIRT_MULTI_GATHER=copy gathers with peer-to-peer
// hipMemcpyAsync instead; a device may then be listed more than once (several parts time-sharing one GPU: a rehearsal of the
// N > 1 code path on a one-GPU box, never a scaling measurement).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mirt.h"
#include "dev_mem.h"
#include "host_scene.h"

namespace {

struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

bool load_rccl(Rccl& r)
{
  for (const char* name : {"librccl.so.1", "librccl.so"}) {
    r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (r.lib) break;
  }
  if (!r.lib) return false;
  r.CommInitAll = (decltype(r.CommInitAll))dlsym(r.lib, "ncclCommInitAll");
  r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
  r.GroupStart = (decltype(r.GroupStart))dlsym(r.lib, "ncclGroupStart");
  r.GroupEnd = (decltype(r.GroupEnd))dlsym(r.lib, "ncclGroupEnd");
  r.Send = (decltype(r.Send))dlsym(r.lib, "ncclSend");
  r.Recv = (decltype(r.Recv))dlsym(r.lib, "ncclRecv");
  r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
  return r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.GetErrorString;
}

// The handles are grouped by the device they live on, in dev_mem.h's owning types; each group makes its device current in its
// destructor's body, which runs before its members go.  What one frame in flight holds on one device:
struct SlotDev {
  int dev = 0;
  mirt::Stream stream;                       // this slot's render stream
  mirt::Event ev0, ev1;                      // part render start / end
  mirt::Event sent;                          // its share of the gather has left (communication stream)
  mirt::DevBuf<unsigned char> part;          // its compact part buffer
  ~SlotDev() { hipSetDevice(dev); }
};

// ... and on device 0 alone
struct SlotRoot {
  int dev = 0;
  std::vector<mirt::DevBuf<unsigned char>> gathered;      // where part r arrives (r >= 1)
  mirt::DevBuf<unsigned char> frame;         // the row-major frame
  mirt::Event gather_end;                    // (communication stream) frame re-interleaved
  mirt::Event done;                          // host copy issued too
  ~SlotRoot() { hipSetDevice(dev); }
};

// everything one frame in flight owns
struct Slot {
  std::vector<SlotDev> on;                   // per device
  SlotRoot at0;
  bool busy = false;
  unsigned long long ticket = 0;
  std::chrono::steady_clock::time_point t0;
};

// what the object holds on one device, whatever the frame
struct PerDev {
  int dev = 0;
  MirtScene* scene = nullptr;                // opaque here: given back through mirt_scene_destroy (mirt_multi_destroy)
  mirt::Stream comm_stream;                  // the gathers, in submission order
  ~PerDev() { hipSetDevice(dev); }
};

} // namespace

// All vectors of n elements are sized once, in mirt_multi_create before the build threads start; nothing resizes them later.
struct MirtMulti {
  int n = 0;
  bool copy_gather = false;                  // peer-to-peer copies instead of RCCL (MIRT_MULTI_GATHER=copy)
  std::vector<int> dev;
  std::vector<PerDev> per;
  Slot slot[MIRT_MULTI_MAX_IN_FLIGHT];
  unsigned long long next_ticket = 1;
  int outstanding = 0;
  Rccl rccl;
  std::vector<ncclComm_t> comm;              // empty unless ncclCommInitAll made them; released through `rccl` (mirt_multi_destroy)
  float build_ms_max = 0.0f;
};

namespace {

// wait for everything the slot has in flight (error paths, reuse, destroy; a stream never made is the device's null stream)
void drain_slot(MirtMulti* mm, Slot& s)
{
  for (int r = 0; r < mm->n; ++r) {
    hipSetDevice(mm->dev[r]);
    hipStreamSynchronize(s.on[r].stream);
    hipStreamSynchronize(mm->per[r].comm_stream);
  }
}

// Overflowed capacities on any device (a full pending-ray list: the image misses contributions)?  mirt_get_stats waits for
// every frame in flight of a scene, so this is only called once the pipeline is empty.
int check_overflow(MirtMulti* mm)
{
  int rc = MIRT_OK;
  for (int r = 0; r < mm->n; ++r) {
    MirtStats st;
    const int q = mirt_get_stats(mm->per[r].scene, &st);
    if (q != MIRT_OK && rc == MIRT_OK) rc = q;      // (the message of the first failing device stays in mirt_last_error)
  }
  return rc;
}

// One device's share of mirt_multi_create, on that device's thread: its scene, streams and events, then its tree.
int create_on_device(MirtMulti* mm, const MirtSceneDesc* desc, int r, float* build_ms)
{
  PerDev& d = mm->per[r];
  MIRT_TRY(mirt_scene_create(desc, d.dev, &d.scene));
  MIRT_HIP(hipSetDevice(d.dev));
  MIRT_TRY(d.comm_stream.create(hipStreamNonBlocking));
  for (Slot& s : mm->slot) {
    SlotDev& q = s.on[r];
    MIRT_TRY(q.stream.create(hipStreamNonBlocking));
    MIRT_TRY(q.ev0.create()); MIRT_TRY(q.ev1.create()); MIRT_TRY(q.sent.create());
    if (r == 0) { MIRT_TRY(s.at0.gather_end.create()); MIRT_TRY(s.at0.done.create()); }
  }
  return mirt_build_lbvh(d.scene, mm->slot[0].on[r].stream, build_ms);
}

} // namespace

extern "C" {

int mirt_multi_num_parts(const MirtMulti* mm) { return mm ? mm->n : 0; }

void mirt_multi_destroy(MirtMulti* mm)
{
  if (!mm) return;
  for (Slot& s : mm->slot) drain_slot(mm, s);
  // the communicators go before the streams they were used on, through the run-time-loaded table
  for (size_t r = 0; r < mm->comm.size(); ++r) { hipSetDevice(mm->dev[r]); mm->rccl.CommDestroy(mm->comm[r]); }
  for (PerDev& d : mm->per) mirt_scene_destroy(d.scene);      // (a scene never made is null, which that call accepts; it waits for the device)
  delete mm;                                                  // streams, events and buffers: the members' destructors
}

int mirt_multi_create(const MirtSceneDesc* desc, int ngpu, const int* devices, MirtMulti** out)
{
  if (!desc || !out || ngpu < 1 || ngpu > MIRT_MULTI_MAX_GPUS) { mirt::set_error("mirt_multi_create: bad argument"); return MIRT_ERR_ARG; }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { mirt::set_error("mirt_multi_create: no HIP device available (libmirt has no CPU path)"); return MIRT_ERR_NO_DEVICE; }
  const char* g = getenv("MIRT_MULTI_GATHER");
  const bool copy_gather = g && strcmp(g, "copy") == 0;
  if (ngpu > ndev && !copy_gather) { mirt::set_error("mirt_multi_create: more GPUs requested than present"); return MIRT_ERR_ARG; }
  std::vector<int> dev;
  for (int r = 0; r < ngpu; ++r) {
    const int d = devices ? devices[r] : (copy_gather ? r % ndev : r);      // (rehearsal: more parts than GPUs time-share them)
    if (d < 0 || d >= ndev) { mirt::set_error("mirt_multi_create: bad device index"); return MIRT_ERR_ARG; }
    // (RCCL refuses a device listed twice; with peer copies several parts may time-share one GPU: a rehearsal, see above)
    if (!copy_gather) for (int q = 0; q < r; ++q) if (dev[q] == d) { mirt::set_error("mirt_multi_create: a device is listed twice"); return MIRT_ERR_ARG; }
    dev.push_back(d);
  }
  MirtMulti* mm = new MirtMulti();
  mm->n = ngpu;
  mm->copy_gather = copy_gather;
  mm->dev = dev;
  mm->per = std::vector<PerDev>(ngpu);
  for (Slot& s : mm->slot) { s.on = std::vector<SlotDev>(ngpu); s.at0.gathered.resize(ngpu); s.at0.dev = dev[0]; }
  for (int r = 0; r < ngpu; ++r) { mm->per[r].dev = dev[r]; for (Slot& s : mm->slot) s.on[r].dev = dev[r]; }
  // The BVH is replicated: every device gets the same arrays and builds the same tree -- all devices at once, one host thread
  // each (upload and build are synchronous calls, lbvh_builder.cu:475).
  std::vector<int> rcs(ngpu, MIRT_OK);
  std::vector<std::string> msgs(ngpu);
  std::vector<float> bms(ngpu, 0.0f);
  {
    std::vector<std::thread> th;
    for (int r = 0; r < ngpu; ++r) {
      th.emplace_back([&, r]() {
        rcs[r] = create_on_device(mm, desc, r, &bms[r]);
        if (rcs[r] != MIRT_OK) msgs[r] = mirt_last_error();      // (the error string is per thread)
      });
    }
    for (std::thread& t : th) t.join();
  }
  for (int r = 0; r < ngpu; ++r) {
    if (rcs[r] != MIRT_OK) { const int rc = rcs[r]; const std::string m = msgs[r]; mirt_multi_destroy(mm); mirt::set_error(m); return rc; }
    if (bms[r] > mm->build_ms_max) mm->build_ms_max = bms[r];
  }
  if (ngpu > 1 && !copy_gather) {
    if (!load_rccl(mm->rccl)) { mirt_multi_destroy(mm); mirt::set_error("mirt_multi_create: librccl.so not found (needed for more than one GPU)"); return MIRT_ERR_STATE; }
    std::vector<ncclComm_t> comm(ngpu, nullptr);
    ncclResult_t nr = mm->rccl.CommInitAll(comm.data(), ngpu, mm->dev.data());
    if (nr != ncclSuccess) {
      std::string msg = std::string("mirt_multi_create: ncclCommInitAll: ") + mm->rccl.GetErrorString(nr);
      mirt_multi_destroy(mm); mirt::set_error(msg); return MIRT_ERR_HIP;
    }
    mm->comm = std::move(comm);
  }
  *out = mm;
  return MIRT_OK;
}

int mirt_multi_set_option(MirtMulti* mm, const char* name, int value)
{
  if (!mm) { mirt::set_error("mirt_multi_set_option: null argument"); return MIRT_ERR_ARG; }
  for (PerDev& d : mm->per) { int rc = mirt_scene_set_option(d.scene, name, value); if (rc != MIRT_OK) return rc; }
  return MIRT_OK;
}

int mirt_multi_set_camera(MirtMulti* mm, const MirtCamera* cam)
{
  if (!mm || !cam) { mirt::set_error("mirt_multi_set_camera: null argument"); return MIRT_ERR_ARG; }
  for (PerDev& d : mm->per) { int rc = mirt_scene_set_camera(d.scene, cam); if (rc != MIRT_OK) return rc; }
  return MIRT_OK;
}

// The scene's setter on every device, on that device's default stream, and the records in place before the call returns: the
// frames submitted afterwards run on the slots' own (non-blocking) streams, which no stream order ties to this one.
int mirt_multi_set_lights(MirtMulti* mm, const MirtLight* suns, const MirtLight* bulbs)
{
  if (!mm) { mirt::set_error("mirt_multi_set_lights: null argument"); return MIRT_ERR_ARG; }
  for (PerDev& d : mm->per) {
    int rc = mirt_scene_set_lights(d.scene, suns, bulbs, nullptr);
    if (rc != MIRT_OK) return rc;
    MIRT_HIP(hipStreamSynchronize(nullptr));
  }
  return MIRT_OK;
}

int mirt_multi_set_planes(MirtMulti* mm, const MirtPlane* planes, int first, int count)
{
  if (!mm) { mirt::set_error("mirt_multi_set_planes: null argument"); return MIRT_ERR_ARG; }
  for (PerDev& d : mm->per) {
    int rc = mirt_scene_set_planes(d.scene, planes, first, count, nullptr);
    if (rc != MIRT_OK) return rc;
    MIRT_HIP(hipStreamSynchronize(nullptr));
  }
  return MIRT_OK;
}

int mirt_multi_set_shading(MirtMulti* mm, const MirtShading* sh)
{
  if (!mm || !sh) { mirt::set_error("mirt_multi_set_shading: null argument"); return MIRT_ERR_ARG; }
  for (PerDev& d : mm->per) { int rc = mirt_scene_set_shading(d.scene, sh); if (rc != MIRT_OK) return rc; }
  return MIRT_OK;
}

int mirt_multi_get_stats(MirtMulti* mm, int part, MirtStats* out)
{
  if (!mm || part < 0 || part >= mm->n || !out) { mirt::set_error("mirt_multi_get_stats: bad argument"); return MIRT_ERR_ARG; }
  return mirt_get_stats(mm->per[part].scene, out);
}

static int submit_impl(MirtMulti* mm, Slot& s, int width, int height, int spp, int stripe_rows, uint8_t* host_rgba)
{
  const int n = mm->n;
  std::vector<MirtRenderParams> prm(n);
  std::vector<int64_t> npix(n);
  int64_t maxpix = 0;
  for (int r = 0; r < n; ++r) {
    MirtRenderParams& p = prm[r];
    p.width = width; p.height = height; p.spp = spp; p.stripe_rows = n > 1 ? stripe_rows : height; p.num_parts = n; p.part = r; p.flags = 0;
    npix[r] = mirt_render_num_pixels(&p);
    if (npix[r] < 0) { mirt::set_error("mirt_multi_submit: bad frame parameters"); return MIRT_ERR_ARG; }
    if (npix[r] > maxpix) maxpix = npix[r];
  }
  // buffers of this slot (grown on demand, kept; the slot is idle here)
  const size_t part_bytes = (size_t)maxpix * 4, frame_bytes = (size_t)width * height * 4;
  // The capacity of the LAST part buffer allocated stands for all of them: all are reset before the first is allocated, so a
  // failure midway leaves it 0 and the next submit allocates again.  (part_bytes > 0: part 0 owns row 0 of a frame with pixels.)
  const mirt::DevBuf<unsigned char>& last = n > 1 ? s.at0.gathered[n - 1] : s.on[0].part;
  if (last.cap() < part_bytes) {
    for (int r = 0; r < n; ++r) { s.on[r].part.reset(); s.at0.gathered[r].reset(); }
    for (int r = 0; r < n; ++r) { MIRT_HIP(hipSetDevice(mm->dev[r])); MIRT_TRY(s.on[r].part.alloc(part_bytes)); }
    MIRT_HIP(hipSetDevice(mm->dev[0]));
    for (int r = 1; r < n; ++r) MIRT_TRY(s.at0.gathered[r].alloc(part_bytes));
  }
  if (n > 1 && s.at0.frame.cap() < frame_bytes) {
    MIRT_HIP(hipSetDevice(mm->dev[0]));
    MIRT_TRY(s.at0.frame.alloc(frame_bytes));
  }
  // every device renders its stripes on this slot's stream
  for (int r = 0; r < n; ++r) {
    MIRT_HIP(hipSetDevice(mm->dev[r]));
    MIRT_HIP(hipEventRecord(s.on[r].ev0, s.on[r].stream));
    if (npix[r] > 0) { int rc = mirt_render(mm->per[r].scene, &prm[r], s.on[r].part, nullptr, s.on[r].stream); if (rc != MIRT_OK) return rc; }
    MIRT_HIP(hipEventRecord(s.on[r].ev1, s.on[r].stream));
    MIRT_HIP(hipStreamWaitEvent(mm->per[r].comm_stream, s.on[r].ev1, 0));      // the gather of this frame follows its part, and the gathers before it
  }
  const void* result = s.on[0].part;       // one device: its part is the row-major frame
  if (n > 1) {
    if (mm->copy_gather) {
      // peer-to-peer copies issued on the sender's communication stream; device 0 waits for each
      for (int r = 1; r < n; ++r) {
        if (npix[r] == 0) continue;
        MIRT_HIP(hipSetDevice(mm->dev[r]));
        MIRT_HIP(hipMemcpyPeerAsync(s.at0.gathered[r], mm->dev[0], s.on[r].part, mm->dev[r], (size_t)npix[r] * 4, mm->per[r].comm_stream));
        MIRT_HIP(hipEventRecord(s.on[r].ev1, mm->per[r].comm_stream));
        MIRT_HIP(hipSetDevice(mm->dev[0]));
        MIRT_HIP(hipStreamWaitEvent(mm->per[0].comm_stream, s.on[r].ev1, 0));
      }
    } else {
      // framebuffer gather to device 0: one grouped exchange per frame, each peer on its own xGMI link
      ncclResult_t nr = mm->rccl.GroupStart();
      for (int r = 1; r < n && nr == ncclSuccess; ++r) {
        if (npix[r] == 0) continue;
        nr = mm->rccl.Send(s.on[r].part, (size_t)npix[r] * 4, ncclUint8, 0, mm->comm[r], mm->per[r].comm_stream);
        if (nr == ncclSuccess) nr = mm->rccl.Recv(s.at0.gathered[r], (size_t)npix[r] * 4, ncclUint8, r, mm->comm[0], mm->per[0].comm_stream);
      }
      const ncclResult_t ne = mm->rccl.GroupEnd();
      if (nr == ncclSuccess) nr = ne;
      if (nr != ncclSuccess) { mirt::set_error(std::string("mirt_multi_submit: RCCL: ") + mm->rccl.GetErrorString(nr)); return MIRT_ERR_HIP; }
    }
    for (int r = 1; r < n; ++r) { MIRT_HIP(hipSetDevice(mm->dev[r])); MIRT_HIP(hipEventRecord(s.on[r].sent, mm->per[r].comm_stream)); }
    MIRT_HIP(hipSetDevice(mm->dev[0]));
    for (int r = 0; r < n; ++r) {
      if (npix[r] == 0) continue;
      int rc = mirt_scatter_part(&prm[r], r == 0 ? s.on[0].part : s.at0.gathered[r], s.at0.frame, mm->per[0].comm_stream);
      if (rc != MIRT_OK) return rc;
    }
    result = s.at0.frame;
  }
  MIRT_HIP(hipSetDevice(mm->dev[0]));
  MIRT_HIP(hipEventRecord(s.at0.gather_end, mm->per[0].comm_stream));
  if (host_rgba) MIRT_HIP(hipMemcpyAsync(host_rgba, result, frame_bytes, hipMemcpyDeviceToHost, mm->per[0].comm_stream));
  MIRT_HIP(hipEventRecord(s.at0.done, mm->per[0].comm_stream));
  return MIRT_OK;
}

int mirt_multi_submit(MirtMulti* mm, int width, int height, int spp, int stripe_rows, uint8_t* host_rgba, uint64_t* ticket)
{
  if (!mm || width <= 0 || height <= 0 || spp < 0 || stripe_rows <= 0 || !ticket) { mirt::set_error("mirt_multi_submit: bad argument"); return MIRT_ERR_ARG; }
  Slot& s = mm->slot[mm->next_ticket % MIRT_MULTI_MAX_IN_FLIGHT];
  if (s.busy) { mirt::set_error("mirt_multi_submit: MIRT_MULTI_MAX_IN_FLIGHT frames are in flight: mirt_multi_wait for the oldest first"); return MIRT_ERR_STATE; }
  s.t0 = std::chrono::steady_clock::now();
  const int rc = submit_impl(mm, s, width, height, spp, stripe_rows, host_rgba);
  if (rc != MIRT_OK) {
    // nothing of a half-issued frame stays in flight behind the caller's back
    const std::string msg = mirt_last_error();
    drain_slot(mm, s);
    mirt::set_error(msg);
    return rc;
  }
  s.busy = true;
  s.ticket = mm->next_ticket++;
  ++mm->outstanding;
  *ticket = s.ticket;
  return MIRT_OK;
}

int mirt_multi_wait(MirtMulti* mm, uint64_t ticket, MirtMultiStats* stats)
{
  if (!mm) { mirt::set_error("mirt_multi_wait: null argument"); return MIRT_ERR_ARG; }
  Slot& s = mm->slot[ticket % MIRT_MULTI_MAX_IN_FLIGHT];
  if (!s.busy || s.ticket != ticket) { mirt::set_error("mirt_multi_wait: no such frame in flight"); return MIRT_ERR_ARG; }
  const int n = mm->n;
  for (int r = 0; r < n; ++r) {
    MIRT_HIP(hipSetDevice(mm->dev[r]));
    MIRT_HIP(hipEventSynchronize(s.on[r].ev1));
    if (r > 0 && n > 1) MIRT_HIP(hipEventSynchronize(s.on[r].sent));      // its part buffer is free again
  }
  MIRT_HIP(hipSetDevice(mm->dev[0]));
  MIRT_HIP(hipEventSynchronize(s.at0.done));
  s.busy = false;
  --mm->outstanding;
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->num_gpus = n;
    stats->build_ms = mm->build_ms_max;
    if (!mm->copy_gather || n == 1) {      // (with peer copies ev1[r >= 1] was re-recorded after the copy)
      for (int r = 0; r < n && r < MIRT_MULTI_MAX_GPUS; ++r) {
        MIRT_HIP(hipSetDevice(mm->dev[r]));
        MIRT_HIP(hipEventElapsedTime(&stats->render_ms[r], s.on[r].ev0, s.on[r].ev1));
      }
    } else {
      MIRT_HIP(hipSetDevice(mm->dev[0]));
      MIRT_HIP(hipEventElapsedTime(&stats->render_ms[0], s.on[0].ev0, s.on[0].ev1));
    }
    MIRT_HIP(hipSetDevice(mm->dev[0]));
    MIRT_HIP(hipEventElapsedTime(&stats->gather_ms, s.on[0].ev1, s.at0.gather_end));
    stats->frame_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - s.t0).count();
  }
  // a capacity overflow on any device makes the frame untrustworthy: checked whenever the pipeline is empty
  if (mm->outstanding == 0) return check_overflow(mm);
  return MIRT_OK;
}

int mirt_render_frame_multi(MirtMulti* mm, int width, int height, int spp, int stripe_rows, uint8_t* host_rgba, MirtMultiStats* stats)
{
  uint64_t t = 0;
  int rc = mirt_multi_submit(mm, width, height, spp, stripe_rows, host_rgba, &t);
  if (rc != MIRT_OK) return rc;
  return mirt_multi_wait(mm, t, stats);
}

int mirt_render_frames_multi(MirtMulti* mm, int width, int height, int spp, int stripe_rows, int nframes, int in_flight, uint8_t* host_rgba_last,
                             MirtMultiStats* last_stats, float* ms_per_frame)
{
  if (!mm || nframes < 1 || in_flight < 1 || in_flight > MIRT_MULTI_MAX_IN_FLIGHT) { mirt::set_error("mirt_render_frames_multi: bad argument"); return MIRT_ERR_ARG; }
  if (mm->outstanding != 0) { mirt::set_error("mirt_render_frames_multi: frames of an earlier mirt_multi_submit are still in flight"); return MIRT_ERR_STATE; }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint64_t> tk(nframes, 0);
  int rc = MIRT_OK;
  int issued = 0, waited = 0;
  for (; issued < nframes && rc == MIRT_OK; ++issued) {
    if (issued - waited >= in_flight) { rc = mirt_multi_wait(mm, tk[waited], nullptr); ++waited; if (rc != MIRT_OK) break; }
    rc = mirt_multi_submit(mm, width, height, spp, stripe_rows, issued == nframes - 1 ? host_rgba_last : nullptr, &tk[issued]);
    if (rc != MIRT_OK) break;
  }
  const std::string msg = rc != MIRT_OK ? std::string(mirt_last_error()) : std::string();
  for (; waited < issued; ++waited) {      // drain, whatever happened
    const int q = mirt_multi_wait(mm, tk[waited], waited == nframes - 1 ? last_stats : nullptr);
    if (q != MIRT_OK && rc == MIRT_OK) rc = q;
  }
  if (!msg.empty()) mirt::set_error(msg);
  if (ms_per_frame) *ms_per_frame = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count() / (float)nframes;
  return rc;
}

} // extern "C"
