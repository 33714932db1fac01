"""The reference's plotting/ package, reduced to what writes a number: the ground-truth correlation (GTC) of
representation_plot on the fp64 HIP kernels of csrc/gtc.hip.  No figure is drawn anywhere in this build (the reference's package
initialiser, which picks a matplotlib backend, has nothing to do here)."""
