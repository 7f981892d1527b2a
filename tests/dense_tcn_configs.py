"""The configurations of the causal Conv-TasNet WITHOUT separable convolutions (two full k-tap dilated convolutions per TCN layer, reference
src/models/tdcn.py:100-147) that tests/test_dense_tcn_cpu.py and tests/test_dense_tcn_gpu.py run, and the shapes of their fixtures
tests/golden/convtasnet_<name>.npz -- written by tools/make_dense_tcn_golden.py from the unmodified reference, with the keys
oracle/make_golden.py writes."""

_SHARED = dict(kernel_size=16, stride=8, enc_basis="trainable", dec_basis="trainable", dilated=True, separable=False, causal=True,
               sep_nonlinear="prelu", sep_norm=True)
CONFIGS = {
    # two separate heads products (Bn = 16), dilations 1 / 2 / 4, a last layer without the output head, encoder ReLU, sigmoid mask
    "causal16_dense": dict(_SHARED, n_basis=32, enc_nonlinear="relu", sep_hidden_channels=32, sep_bottleneck_channels=16, sep_skip_channels=16,
                           sep_kernel_size=3, sep_num_blocks=2, sep_num_layers=3, mask_nonlinear="sigmoid", n_sources=2),
    # a 128-row bottleneck: the joint [Wo; Ws] product, contraction length H P = 240, a history of (P - 1) d = 32 frames at the last layer
    "causal16_dense_joint": dict(_SHARED, n_basis=32, enc_nonlinear=None, sep_hidden_channels=48, sep_bottleneck_channels=128, sep_skip_channels=32,
                                 sep_kernel_size=5, sep_num_blocks=1, sep_num_layers=4, mask_nonlinear="softmax", n_sources=3),
}
SHAPES = {"causal16_dense": (2, 2403), "causal16_dense_joint": (3, 1500)}      # (batch, samples)
NAMES = tuple(CONFIGS)
