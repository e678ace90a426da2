"""take_amd — host side of the MI355X path-tracing core behind TaKe's `render()`.

  capi    ctypes binding of the C ABI (include/take_hip.h, take_amd/libtake_hip.so built from csrc/): Scene, SceneGroup,
          and every name of the modules below, which is where callers import the binding from
  image   the binding's scene-free image-space calls (denoisers, temporal accumulation, display transform, bloom)
  meshes  the binding's DeviceMesh, Rig, Subdiv, Displace and the calls on bare meshes
  _lib    loads the library and gives every entry point its prototype;  _marshal: arrays, streams and handles
  cdefs   ctypes mirror of the header's structs and constants, and PROTOTYPES: every entry point's argument types
  scene   SceneData: a flattened reference `Scene` (+ .tkscene files written by take_amd/host/take_flatten.hpp)
  render  the reference's render()/main() convention on top of the C ABI;  exr: its image.exr writer
  dist    row-strip sharding over one process per GPU and the single gather
  scenes  procedural benchmark scenes (BASELINE.json configs)
There is no CPU rendering path in this package: every render call goes to the HIP library and fails without a GPU.
"""
