"""MI355X-native hot path of jgsimard/big-dreamer (Dreamer.train_step) -- see DESIGN.md."""
