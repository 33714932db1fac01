"""Evaluation of a learned representation (reference evaluation/): KNN-MSE on the exact HIP k-nearest-neighbour search
(knn_images) and the states of a trained model on another dataset (predict_dataset).  Plots are out of scope of this build."""
