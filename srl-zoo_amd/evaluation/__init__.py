"""Evaluation of a learned representation (reference evaluation/): KNN-MSE on the exact HIP k-nearest-neighbour search
(knn_images), the states of a trained model on another dataset (predict_dataset), the results table of a folder of
experiments (gather_results), the reward-prediction probe on its one-launch-per-phase kernels (predict_reward) and the
latent-space viewer (enjoy_latent: the reference's window loop on an injectable backend, or headless traversal sheets, the images
made on the GPU by csrc/latent.hip).  Plots are out of scope of this build."""
